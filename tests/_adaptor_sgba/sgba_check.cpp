// Optimizer::LocalBundleAdjustment with its planes and rooms on resident keyframes and map points through
// include/vsg_orb_adaptor.hpp from plain C++: the flat binary file of tests/_adaptor_localba/localba_check.cpp, then the
// planes and rooms (tests/test_gpu_sgraph_local_ba.py writes it); vsg::ResidentMapPoints::LocalBundleAdjustmentSGraph runs
// on them and its result, with the listed slots read back, goes to a second file the test compares with the bytes of the
// Python call.  Without a device the store throws (exit 3).
//   usage: sgba_check <in.bin> <out.bin>
#include <cstdio>
#include <fstream>
#include <memory>

#include "vsg_orb_adaptor.hpp"

template <class T>
static void dump(std::ofstream &f, const std::vector<T> &v) {
  int32_t n = (int32_t)v.size();
  f.write((const char *)&n, 4);
  if (n) f.write((const char *)v.data(), sizeof(T) * v.size());
}
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
    vsg::ResidentMapPoints probe(16);  // no device: throws here ("no CPU fallback")
    std::ifstream in(argv[1], std::ios::binary);
    if (!in) return 2;
    const std::vector<int32_t> head = load<int32_t>(in);  // capacity, iterations, number of keyframes
    if (head.size() != 3 || head[2] < 0) return 2;
    std::vector<std::unique_ptr<vsg::ResidentFrame>> frames;
    std::vector<vsg_frame *> handles;
    for (int k = 0; k < head[2]; ++k) {
      const std::vector<vsg_keypoint> keys = load<vsg_keypoint>(in);
      const std::vector<float> ur = load<float>(in);  // empty: every mvuRight is -1
      const std::vector<uint8_t> desc(32 * keys.size(), 0);
      frames.emplace_back(new vsg::ResidentFrame((int)keys.size() + 1));
      frames.back()->Upload(keys.data(), desc.data(), ur.empty() ? nullptr : ur.data(), (int)keys.size(), -1, 0.0f, 0.0f, 640.0f,
                            480.0f);
      handles.push_back(frames.back()->handle());
    }
    const std::vector<float> pos = load<float>(in);  // the whole store, 3 floats per slot
    const std::vector<int32_t> slots = load<int32_t>(in), off = load<int32_t>(in), kf = load<int32_t>(in), idx = load<int32_t>(in);
    const std::vector<vsg_pose_se3> Tcw = load<vsg_pose_se3>(in);
    const std::vector<uint8_t> fixed = load<uint8_t>(in);
    const std::vector<vsg_ba_camera> cam = load<vsg_ba_camera>(in);
    const std::vector<float> sig = load<float>(in);
    vsg::SGraphLists sg;
    sg.planeEq = load<double>(in), sg.planeObsOff = load<int32_t>(in), sg.planeObsKf = load<int32_t>(in);
    sg.planeObsLocal = load<double>(in), sg.planeObsG = load<double>(in), sg.wPlaneKf = load<double>(in), sg.wPlanePoint = load<double>(in);
    sg.roomCenter = load<double>(in), sg.roomNWalls = load<int32_t>(in), sg.roomWall = load<int32_t>(in);
    if (!in) return 2;
    std::vector<int32_t> all(head[0]);
    for (int i = 0; i < head[0]; ++i) all[i] = i;
    vsg::ResidentMapPoints mp(head[0]);
    mp.update(all, pos.data(), nullptr, nullptr, nullptr, nullptr, nullptr);  // SetWorldPos
    const vsg::SGraphLocalBAResult r = mp.LocalBundleAdjustmentSGraph(slots, off, kf, idx, handles, Tcw, fixed, cam, sig, sg, head[1]);
    std::vector<float> after(3 * (size_t)head[0]);
    vsg::check(vsg_mappoints_read(mp.handle(), head[0], all.data(), after.data(), nullptr, nullptr, nullptr, nullptr, nullptr),
               "vsg_mappoints_read");
    std::ofstream out(argv[2], std::ios::binary);
    dump(out, r.kfTcw), dump(out, r.worldPos), dump(out, r.erase), dump(out, r.chi2), dump(out, r.planeEq), dump(out, r.roomCenter);
    dump(out, r.erasePlane), dump(out, r.chi2PlaneKf), dump(out, r.chi2PlanePoint);
    dump(out, std::vector<vsg_sgraph_local_ba_result>(1, r.res)), dump(out, after);
    printf("OK %d\n", (int)slots.size());
    return 0;
  } catch (const std::exception &e) {
    printf("THROW %s (no CPU fallback)\n", e.what());
    return 3;
  }
}
