// MapPoint::ComputeDistinctiveDescriptors + UpdateNormalAndDepth on resident map points through
// include/vsg_orb_adaptor.hpp from plain C++: keyframes (keypoints, descriptors), map-point positions and observation
// lists come from a flat binary file written by tests/test_abi_observations.py; vsg::ResidentMapPoints::Refresh runs on
// them and its result, with the refreshed slots read back, goes to a second file the test compares with
// tests/observations_reference.py.  Without a device the store throws (exit 3).
//   usage: refresh_check <in.bin> <out.bin>
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
    const std::vector<int32_t> head = load<int32_t>(in);  // capacity, what, number of keyframes
    if (head.size() != 3 || head[2] < 0) return 2;
    std::vector<std::unique_ptr<vsg::ResidentFrame>> frames;
    std::vector<vsg_frame *> handles;
    for (int k = 0; k < head[2]; ++k) {
      const std::vector<vsg_keypoint> keys = load<vsg_keypoint>(in);
      const std::vector<uint8_t> desc = load<uint8_t>(in);
      frames.emplace_back(new vsg::ResidentFrame((int)keys.size() + 1));
      frames.back()->Upload(keys.data(), desc.data(), nullptr, (int)keys.size(), -1, 0.0f, 0.0f, 640.0f, 480.0f);
      handles.push_back(frames.back()->handle());
    }
    const std::vector<float> Ow = load<float>(in), sf = load<float>(in), pos = load<float>(in);
    const std::vector<int32_t> slots = load<int32_t>(in), off = load<int32_t>(in), kf = load<int32_t>(in),
                               idx = load<int32_t>(in), ref = load<int32_t>(in);
    const std::vector<uint8_t> bad = load<uint8_t>(in);  // empty: no keyframe is bad
    if (!in) return 2;
    const int n = (int)slots.size();

    vsg::ResidentMapPoints mp(head[0]);
    mp.update(slots, pos.data(), nullptr, nullptr, nullptr, nullptr, nullptr);  // SetWorldPos
    const vsg::RefreshResult r = mp.Refresh(slots, off, kf, idx, bad, ref, handles, Ow, sf, head[1]);
    std::vector<float> nrm(3 * n), dmin(n), dmax(n);
    std::vector<uint8_t> desc(32 * n);
    vsg::check(vsg_mappoints_read(mp.handle(), n, slots.data(), nullptr, nrm.data(), dmin.data(), dmax.data(), desc.data(),
                                  nullptr),
               "vsg_mappoints_read");
    std::ofstream out(argv[2], std::ios::binary);
    dump(out, r.best), dump(out, r.normal), dump(out, r.minDist), dump(out, r.maxDist);
    dump(out, nrm), dump(out, dmin), dump(out, dmax), dump(out, desc);
    printf("OK %d\n", n);
    return 0;
  } catch (const std::exception &e) {
    printf("THROW %s (no CPU fallback)\n", e.what());
    return 3;
  }
}
