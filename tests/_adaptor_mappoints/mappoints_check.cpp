// Tracking::SearchLocalPoints through include/vsg_orb_adaptor.hpp from plain C++: a frame (keypoints, descriptors,
// mvuRight), a local map and a pose come from a flat binary file written by tests/test_abi_mappoints.py /
// tests/test_gpu_adaptor_mappoints.py; vsg::ResidentMapPoints::update (in two halves, the second through a slot list),
// vsg::ResidentFrame::isInFrustum and ::SearchLocalPoints run on them and their results go to a second file the test
// compares with tests/frustum_reference.py and the Python binding.  Without a device the store throws (exit 3).
//   usage: mappoints_check <in.bin> <out.bin>
#include <cstdio>
#include <fstream>

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
    const std::vector<float> cam = load<float>(in);     // Rcw[9] tcw[3] Ow[3] fx fy cx cy mbf logScaleFactor
    const std::vector<int32_t> head = load<int32_t>(in);  // nLevels, bFarPoints
    const std::vector<float> par = load<float>(in);     // bounds[4], th, nnratio, thFarPoints
    const std::vector<float> sf = load<float>(in);      // mvScaleFactors
    const std::vector<vsg_keypoint> keys = load<vsg_keypoint>(in);
    const std::vector<uint8_t> desc = load<uint8_t>(in);
    const std::vector<float> uRight = load<float>(in);  // empty: a frame without mvuRight
    const std::vector<float> pos = load<float>(in), nrm = load<float>(in), dmin = load<float>(in), dmax = load<float>(in);
    const std::vector<uint8_t> mdesc = load<uint8_t>(in), obs = load<uint8_t>(in), skip = load<uint8_t>(in);
    if (cam.size() != 21 || head.size() != 2 || par.size() != 7 || !in) return 2;
    const int n = (int)dmin.size();

    vsg::FramePose pose;
    for (int i = 0; i < 9; ++i) pose.Rcw[i] = cam[i];
    for (int i = 0; i < 3; ++i) pose.tcw[i] = cam[9 + i], pose.Ow[i] = cam[12 + i];
    pose.fx = cam[15], pose.fy = cam[16], pose.cx = cam[17], pose.cy = cam[18], pose.mbf = cam[19];
    pose.log_scale_factor = cam[20], pose.n_levels = head[0];

    vsg::ResidentFrame F((int)keys.size() + 1);
    F.Upload(keys.data(), desc.data(), uRight.empty() ? nullptr : uRight.data(), (int)keys.size(), -1, par[0], par[1], par[2],
             par[3]);
    // the local map lives in slots 2 i + 1 of a store twice its size; first everything but the descriptors, then those
    vsg::ResidentMapPoints mp(2 * n + 1);
    std::vector<int32_t> slots(n);
    for (int i = 0; i < n; ++i) slots[i] = 2 * i + 1;
    mp.update(slots, pos.data(), nrm.data(), dmin.data(), dmax.data(), nullptr, obs.data());
    mp.update(slots, nullptr, nullptr, nullptr, nullptr, mdesc.data(), nullptr);

    vsg::FrustumResult fr;
    F.isInFrustum(mp, n, slots.data(), pose, 0.5f, fr);
    vsg::LocalPointsResult lp;
    std::vector<uint8_t> blocked(keys.size(), 0);
    const int nm = F.SearchLocalPoints(mp, n, slots.data(), skip.empty() ? nullptr : skip.data(), pose, par[4], par[5],
                                       head[1] != 0, par[6], sf, blocked, lp);
    std::ofstream out(argv[2], std::ios::binary);
    dump(out, std::vector<int32_t>{nm, lp.nToMatch, mp.capacity(), F.N()});
    dump(out, fr.inView), dump(out, fr.projX), dump(out, fr.projY), dump(out, fr.projXR), dump(out, fr.depth);
    dump(out, fr.scaleLevel), dump(out, fr.viewCos);
    dump(out, lp.trainMatch), dump(out, blocked), dump(out, lp.inView), dump(out, lp.projX), dump(out, lp.projY);
    printf("OK %d %d\n", nm, lp.nToMatch);
    return 0;
  } catch (const std::exception &e) {
    printf("THROW %s (no CPU fallback)\n", e.what());
    return 3;
  }
}
