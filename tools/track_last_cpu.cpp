// The caller-side half of SearchByProjection(CurrentFrame, LastFrame) without resident map points, for
// tools/track_last_probe.py: the projection loop of ORBmatcher.cc:1686-1715 on the host (the kernel's own arithmetic,
// visual_sgraphs_amd/csrc/vsg_project.h, compiled -O2, one thread) and the gather of what
// vsg_frame_search_by_projection_last takes, compacted to the projected points.
#include <string.h>

#include "vsg_project.h"

extern "C" int tl_host_side(const vsg_frame_pose *pose, const float *bounds /* minX, minY, maxX, maxY */, int n,
                            const int32_t *slots, const vsg_keypoint *last_kps, const float *world_pos,
                            const uint8_t *desc, const uint8_t *observed, int32_t *index, uint8_t *q_desc,
                            uint8_t *q_observed, float *u, float *v, float *ur, int32_t *octave, float *angle) {
  const vsg::ImageBounds b = {bounds[0], bounds[2], bounds[1], bounds[3]};
  int m = 0;
  for (int i = 0; i < n; i++) {
    const int s = slots[i];
    if (s < 0) continue;  // no map point, or an outlier
    const vsg::ProjectOut o = vsg::project_last_point(*pose, b, world_pos + 3 * (size_t)s);
    if (!o.valid) continue;
    index[m] = i, u[m] = o.u, v[m] = o.v, ur[m] = o.ur;
    octave[m] = last_kps[i].octave, angle[m] = last_kps[i].angle;
    memcpy(q_desc + 32 * (size_t)m, desc + 32 * (size_t)s, 32);
    q_observed[m] = observed[s];
    m++;
  }
  return m;
}
