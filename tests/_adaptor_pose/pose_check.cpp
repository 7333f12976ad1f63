// Optimizer::PoseOptimization on a resident frame through include/vsg_orb_adaptor.hpp from plain C++: the frame, the
// map points, the slots, the pose and the set the plane step removes come from a flat binary file written by
// tests/test_gpu_pose_optimization.py; vsg::ResidentFrame::PoseOptimization runs with the hold, PoseOptimizationResume
// finishes it, and the result goes to a second file the test compares with the ctypes path byte for byte.
//   usage: pose_check <in.bin> <out.bin>
#include <cstdio>
#include <fstream>

#include "vsg_orb_adaptor.hpp"

template <class T>
static std::vector<T> load(std::ifstream &f) {
  int32_t n = 0;
  f.read((char *)&n, 4);
  std::vector<T> v(n > 0 ? n : 0);
  if (n > 0) f.read((char *)v.data(), sizeof(T) * v.size());
  return v;
}

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  try {
    std::ifstream in(argv[1], std::ios::binary);
    if (!in) return 2;
    const std::vector<int32_t> head = load<int32_t>(in);  // capacity of the store
    const std::vector<uint8_t> keybytes = load<uint8_t>(in);
    const std::vector<float> uRight = load<float>(in), pos = load<float>(in);
    const std::vector<int32_t> featSlots = load<int32_t>(in);
    const std::vector<float> pose = load<float>(in), cam = load<float>(in), sigma = load<float>(in);
    const std::vector<uint8_t> removed = load<uint8_t>(in);
    if (!in || head.size() != 1 || pose.size() != 7 || cam.size() != 5) return 2;
    const int n = (int)(keybytes.size() / sizeof(vsg_keypoint));
    const std::vector<uint8_t> desc((size_t)n * 32, 0);
    vsg::ResidentFrame F(n + 1);
    F.Upload((const vsg_keypoint *)keybytes.data(), desc.data(), uRight.data(), n, -1, 0.0f, 0.0f, 640.0f, 480.0f);
    vsg::ResidentMapPoints mp(head[0]);
    std::vector<int32_t> all(head[0]);
    for (int i = 0; i < head[0]; ++i) all[i] = i;
    mp.update(all, pos.data(), nullptr, nullptr, nullptr, nullptr, nullptr);
    vsg_pose_se3 Tcw;
    for (int k = 0; k < 4; ++k) Tcw.q[k] = pose[k];
    for (int k = 0; k < 3; ++k) Tcw.t[k] = pose[4 + k];
    std::vector<uint8_t> outlier(n, 0);  // mvbOutlier
    vsg::ResidentFrame::PoseOptResult out;
    int ret = F.PoseOptimization(mp, featSlots, Tcw, cam.data(), sigma, outlier, out, true);
    const int32_t held = out.held ? 1 : 0;
    if (out.held) ret = F.PoseOptimizationResume(&removed, outlier, out);  // the plane step ran on out.qd / out.td
    std::ofstream o(argv[2], std::ios::binary);
    const int32_t h[5] = {ret, out.nInitialCorrespondences, out.nBad, out.roundsRun, held};
    o.write((const char *)h, sizeof(h));
    o.write((const char *)outlier.data(), n);
    o.write((const char *)out.q, 16), o.write((const char *)out.t, 12);
    return o ? 0 : 2;
  } catch (const std::exception &e) {
    fprintf(stderr, "pose_check: %s\n", e.what());
    return 3;
  }
}
