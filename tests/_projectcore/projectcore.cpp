// Host build of the projection geometry of the motion-model and relocalisation searches (vsg_project.h), for
// tests/test_projection_reference.py: the same source k_project_points compiles, against the NumPy restatement.
#include "vsg_project.h"

extern "C" {

// vsg::project_last_point for n points; bounds = minX, minY, maxX, maxY; active == nullptr: every point
void pc_project_last(const vsg_frame_pose *pose, const float *bounds, int n, const float *world_pos,
                     const uint8_t *active, uint8_t *valid, float *u, float *v, float *ur) {
  const vsg::ImageBounds b = {bounds[0], bounds[2], bounds[1], bounds[3]};
  for (int i = 0; i < n; i++) {
    vsg::ProjectOut o = {0, 0.0f, 0.0f, 0.0f, 0};
    if (!active || active[i]) o = vsg::project_last_point(*pose, b, world_pos + 3 * i);
    valid[i] = (uint8_t)o.valid, u[i] = o.u, v[i] = o.v, ur[i] = o.ur;
  }
}

// vsg::project_kf_point for n points; skip == nullptr: none
void pc_project_kf(const vsg_frame_pose *pose, const float *bounds, int n, const float *world_pos, const float *min_dist,
                   const float *max_dist, const uint8_t *skip, uint8_t *valid, float *u, float *v, int32_t *level) {
  const vsg::ImageBounds b = {bounds[0], bounds[2], bounds[1], bounds[3]};
  for (int i = 0; i < n; i++) {
    vsg::ProjectOut o = {0, 0.0f, 0.0f, 0.0f, 0};
    if (!(skip && skip[i])) o = vsg::project_kf_point(*pose, b, world_pos + 3 * i, min_dist[i], max_dist[i]);
    valid[i] = (uint8_t)o.valid, u[i] = o.u, v[i] = o.v, level[i] = o.level;
  }
}

int pc_motion_direction(const vsg_frame_pose *cur, const vsg_frame_pose *last, float mb, int mono) {
  return vsg::motion_direction(*cur, *last, mb, mono);
}
}
