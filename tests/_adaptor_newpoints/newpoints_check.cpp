// One neighbour of LocalMapping::CreateNewMapPoints on resident keyframes through include/vsg_orb_adaptor.hpp from plain C++:
// the two keyframes, their stereo values, host FeatureVectors, F12, the epipole, the parameters and the free-slot list come
// from a flat binary file written by tests/test_abi_create_new_map_points.py; vsg::ResidentMatcher::CreateNewMapPoints runs,
// then ResidentMatcher::TriangulateMatches on the matches it returned into a second store, and both results with both
// stores' slots go to a second file the test compares with the ctypes path byte for byte.
//   usage: newpoints_check <in.bin> <out.bin>
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
template <class T>
static void save(std::ofstream &o, const std::vector<T> &v) {
  o.write((const char *)v.data(), sizeof(T) * v.size());
}

struct KeyFrameIn {
  std::vector<uint8_t> keys, desc, noMp;
  std::vector<float> uRight, x3Dc, cosParallax;
  vsg::FeatureVectorCSR fv;
  int n() const { return (int)(keys.size() / sizeof(vsg_keypoint)); }
  void read(std::ifstream &in) {
    keys = load<uint8_t>(in), desc = load<uint8_t>(in), uRight = load<float>(in), x3Dc = load<float>(in);
    cosParallax = load<float>(in), noMp = load<uint8_t>(in);
    fv.node = load<int32_t>(in), fv.off = load<int32_t>(in), fv.idx = load<int32_t>(in);
  }
};

static void dump(std::ofstream &o, const vsg::NewMapPointsResult &r, int n, vsg::ResidentMapPoints &mp, int capacity) {
  const int32_t h[3] = {r.nMatches, r.nCreated, (int32_t)r.vMatchedIndices.size()};
  o.write((const char *)h, sizeof h);
  std::vector<int32_t> pairs;
  for (const auto &p : r.vMatchedIndices) pairs.push_back((int32_t)p.first), pairs.push_back((int32_t)p.second);
  save(o, pairs);
  o.write((const char *)r.reason.data(), n), o.write((const char *)r.source.data(), n);
  o.write((const char *)r.x3D.data(), 12 * (size_t)n), o.write((const char *)r.newSlot.data(), 4 * (size_t)n);
  std::vector<int32_t> all(capacity);
  for (int i = 0; i < capacity; ++i) all[i] = i;
  std::vector<float> pos(3 * (size_t)capacity), nrm(3 * (size_t)capacity), mn(capacity), mx(capacity);
  std::vector<uint8_t> desc(32 * (size_t)capacity), obs(capacity);
  vsg::check(vsg_mappoints_read(mp.handle(), capacity, all.data(), pos.data(), nrm.data(), mn.data(), mx.data(), desc.data(),
                                obs.data()),
             "vsg_mappoints_read");
  save(o, pos), save(o, nrm), save(o, mn), save(o, mx), save(o, desc), save(o, obs);
}

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  try {
    if (vsg_device_count() <= 0) {
      printf("no HIP device: vsg::ResidentMatcher::CreateNewMapPoints has no CPU fallback\n");
      return 3;
    }
    std::ifstream in(argv[1], std::ios::binary);
    if (!in) return 2;
    KeyFrameIn k1, k2;
    k1.read(in), k2.read(in);
    const std::vector<float> F12 = load<float>(in), ep = load<float>(in), sf = load<float>(in), sigma2 = load<float>(in);
    const std::vector<uint8_t> params = load<uint8_t>(in);
    const std::vector<int32_t> freeSlots = load<int32_t>(in), head = load<int32_t>(in);  // head = {capacity}
    if (!in || F12.size() != 9 || ep.size() != 2 || params.size() != sizeof(vsg_triangulation_params) || head.size() != 1) return 2;
    vsg_triangulation_params P;
    memcpy(&P, params.data(), sizeof P);
    const int n1 = k1.n(), n2 = k2.n(), cap = head[0];
    vsg::ResidentFrame A(n1 + 1), B(n2 + 1);
    A.Upload((const vsg_keypoint *)k1.keys.data(), k1.desc.data(), k1.uRight.data(), n1, -1, 0.0f, 0.0f, 320.0f, 240.0f);
    B.Upload((const vsg_keypoint *)k2.keys.data(), k2.desc.data(), k2.uRight.data(), n2, -1, 0.0f, 0.0f, 320.0f, 240.0f);
    A.SetStereoPoints(k1.x3Dc, k1.cosParallax), B.SetStereoPoints(k2.x3Dc, k2.cosParallax);
    vsg::ResidentMapPoints fused(cap), listed(cap);
    vsg::ResidentMatcher matcher(0.6f, true);
    vsg::NewMapPointsResult r1, r2;
    matcher.CreateNewMapPoints(A, k1.noMp.data(), B, k2.noMp.data(), F12.data(), ep.data(), false, false, P, sf, sigma2, sf, sigma2,
                               &fused, freeSlots, r1, &k1.fv, &k2.fv);
    std::vector<int32_t> m12(n1, -1);
    for (const auto &p : r1.vMatchedIndices) m12[p.first] = (int32_t)p.second;
    matcher.TriangulateMatches(A, B, m12, P, sf, sigma2, sf, sigma2, &listed, freeSlots, r2);
    std::ofstream o(argv[2], std::ios::binary);
    dump(o, r1, n1, fused, cap), dump(o, r2, n1, listed, cap);
    if (!o) return 2;
    printf("OK %d matches, %d points\n", r1.nMatches, r1.nCreated);
    return 0;
  } catch (const std::exception &e) {
    fprintf(stderr, "newpoints_check: %s\n", e.what());
    return 3;
  }
}
