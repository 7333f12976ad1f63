// Optimizer::OptimizeSim3 on resident keyframes and map points through include/vsg_orb_adaptor.hpp from plain C++: one
// scene of tests/sim3opt_scenes.py comes from a flat binary file written by tests/test_gpu_sim3_optimization.py (blocks of
// int32 count + data); vsg::ResidentSim3Optimizer runs the call of LoopClosing.cc:538 and what it leaves behind -- the
// return value, nBad, the nulled matches, g2oS12 and mAcumHessian -- goes to a second file the test compares with the
// device call's bytes.
//   usage: sim3opt_check <in.bin> <out.bin>
#include <cstdio>
#include <cstring>
#include <fstream>

#include "vsg_orb_adaptor.hpp"

template <class T>
static std::vector<T> block(std::ifstream &f) {
  int32_t n = 0;
  f.read((char *)&n, 4);
  std::vector<T> v((size_t)(n > 0 ? n : 0));
  if (n > 0) f.read((char *)v.data(), sizeof(T) * (size_t)n);
  return v;
}

static vsg::FramePose pose_of(const std::vector<float> &p) {  // Rcw[9], tcw[3], fx, fy, cx, cy
  vsg::FramePose o;
  memset(&o, 0, sizeof o);
  memcpy(o.Rcw, p.data(), 36), memcpy(o.tcw, p.data() + 9, 12);
  o.fx = p[12], o.fy = p[13], o.cx = p[14], o.cy = p[15];
  return o;
}

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  try {
    if (vsg_device_count() <= 0) {
      printf("no HIP device: vsg::ResidentSim3Optimizer has no CPU fallback\n");
      return 3;
    }
    std::ifstream in(argv[1], std::ios::binary);
    if (!in) return 2;
    const std::vector<int32_t> head = block<int32_t>(in);  // cap1, cap2, fix_scale, all_points
    const std::vector<uint8_t> k1 = block<uint8_t>(in), k2 = block<uint8_t>(in);
    const std::vector<float> pos1 = block<float>(in), pos2 = block<float>(in);
    const std::vector<int32_t> slots1 = block<int32_t>(in), slots2 = block<int32_t>(in), idx2 = block<int32_t>(in),
                               level2 = block<int32_t>(in);
    const std::vector<float> p1 = block<float>(in), p2 = block<float>(in), sig1 = block<float>(in), sig2 = block<float>(in);
    const std::vector<double> S = block<double>(in);
    const std::vector<float> th2 = block<float>(in);
    if (!in || head.size() != 4 || p1.size() != 16 || p2.size() != 16 || S.size() != 8 || th2.size() != 1) return 2;
    const int n1 = (int)(k1.size() / sizeof(vsg_keypoint)), n2 = (int)(k2.size() / sizeof(vsg_keypoint));
    const std::vector<uint8_t> d1((size_t)n1 * 32, 0), d2((size_t)n2 * 32, 0);
    vsg::ResidentFrame kf1(n1 + 1), kf2(n2 + 1);
    kf1.Upload((const vsg_keypoint *)k1.data(), d1.data(), nullptr, n1, -1, 0.0f, 0.0f, 640.0f, 480.0f);
    kf2.Upload((const vsg_keypoint *)k2.data(), d2.data(), nullptr, n2, -1, 0.0f, 0.0f, 640.0f, 480.0f);
    vsg::ResidentMapPoints mp1(head[0]), mp2(head[1]);
    std::vector<int32_t> all1((size_t)head[0]), all2((size_t)head[1]);
    for (size_t i = 0; i < all1.size(); ++i) all1[i] = (int32_t)i;
    for (size_t i = 0; i < all2.size(); ++i) all2[i] = (int32_t)i;
    mp1.update(all1, pos1.data(), nullptr, nullptr, nullptr, nullptr, nullptr);
    mp2.update(all2, pos2.data(), nullptr, nullptr, nullptr, nullptr, nullptr);
    vsg::ResidentSim3Optimizer opt(kf1, kf2, mp1, mp2, pose_of(p1), pose_of(p2), sig1, sig2);
    vsg_sim3d gScm;
    memcpy(gScm.q, S.data(), 32), memcpy(gScm.t, S.data() + 4, 24), gScm.s = S[7];
    double mHessian7x7[49];
    for (double &v : mHessian7x7) v = 1.0;
    std::vector<uint8_t> nulled;
    const int numOptMatches = opt.OptimizeSim3(slots1, slots2, idx2, level2, nulled, gScm, th2[0], head[2] != 0, mHessian7x7,
                                               head[3] != 0);
    std::ofstream o(argv[2], std::ios::binary);
    const int32_t h[2] = {numOptMatches, opt.result().n_bad};
    o.write((const char *)h, sizeof h);
    o.write((const char *)nulled.data(), (std::streamsize)nulled.size());
    o.write((const char *)&gScm, sizeof gScm);
    o.write((const char *)mHessian7x7, sizeof mHessian7x7);
    if (!o) return 2;
    printf("OK %d matches after the optimisation, %d bad\n", numOptMatches, opt.result().n_bad);
    return 0;
  } catch (const std::exception &e) {
    fprintf(stderr, "sim3opt_check: %s\n", e.what());
    return 3;
  }
}
