// Stand-alone driver of the host core (keyframecore.cpp: vsg::project_keyframe_point, vsg::keyframe_bounds) for
// tests/test_sanitizers_keyframe.py, built with AddressSanitizer + UndefinedBehaviorSanitizer linked in.
//   keyframe_sanitized IN OUT
// IN holds records [int32 n, has_skip, sizeof(vsg_frame_pose) | pose | bounds minX minY maxX maxY | world_pos 3n | normal 3n |
// min_dist n | max_dist n | skip n (has_skip)] until its end; OUT gets [valid n (u8) | u n | v n | ur n | level n (i32) |
// the truncated bounds 4] per record.  Every array is a heap block of exactly its size, so a step past an end is reported.
#include <cstdio>
#include <vector>

#include "vsg_project.h"

extern "C" {
void kc_project_keyframe(const vsg_frame_pose *pose, const float *bounds, int n, const float *world_pos,
                         const float *normal, const float *min_dist, const float *max_dist, const uint8_t *skip,
                         uint8_t *valid, float *u, float *v, float *ur, int32_t *level);
void kc_keyframe_bounds(const float *bounds, float *out);
}

template <class T>
static bool get(FILE *f, std::vector<T> &a) {
  return a.empty() || fread(a.data(), sizeof(T), a.size(), f) == a.size();
}
template <class T>
static bool put(FILE *f, const std::vector<T> &a) {
  return a.empty() || fwrite(a.data(), sizeof(T), a.size(), f) == a.size();
}

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int32_t head[3];
  while (fread(head, sizeof(head), 1, in) == 1) {
    if (head[0] < 0 || head[2] != (int32_t)sizeof(vsg_frame_pose)) return 3;
    const size_t n = (size_t)head[0];
    std::vector<vsg_frame_pose> pose(1);
    std::vector<float> bounds(4), P(3 * n), Pn(3 * n), mn(n), mx(n), u(n), v(n), ur(n), kf(4);
    std::vector<uint8_t> skip(head[1] ? n : 0), valid(n);
    std::vector<int32_t> level(n);
    if (!get(in, pose) || !get(in, bounds) || !get(in, P) || !get(in, Pn) || !get(in, mn) || !get(in, mx) || !get(in, skip))
      return 3;
    kc_project_keyframe(pose.data(), bounds.data(), head[0], P.data(), Pn.data(), mn.data(), mx.data(),
                        head[1] ? skip.data() : nullptr, valid.data(), u.data(), v.data(), ur.data(), level.data());
    kc_keyframe_bounds(bounds.data(), kf.data());
    if (!put(out, valid) || !put(out, u) || !put(out, v) || !put(out, ur) || !put(out, level) || !put(out, kf)) return 4;
  }
  return fclose(out) == 0 && fclose(in) == 0 ? 0 : 4;
}
