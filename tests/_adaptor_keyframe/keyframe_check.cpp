// Fuse x2 and the Sim3 projection search on resident map points through include/vsg_orb_adaptor.hpp from plain C++: the
// two vsg::ResidentMatcher::Fuse overloads and the SearchByProjection overload that take a ResidentMapPoints store plus
// slots.  A target KeyFrame, a pose, a map and its skip flags come from a flat binary file written by
// tests/test_abi_keyframe_points.py; the results go to a second file the test compares with the Python binding and the
// reference.  Without a device the store throws (exit 3).
//   usage: keyframe_check <in.bin> <out.bin>
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
    const std::vector<float> cam = load<float>(in);      // Rcw[9] tcw[3] Ow[3] fx fy cx cy mbf logScaleFactor
    const std::vector<int32_t> head = load<int32_t>(in);  // nLevels, th of the Sim3 search
    const std::vector<float> par = load<float>(in);       // bounds[4], th (Fuse), th (Sim3 Fuse), ratioHamming
    const std::vector<float> sf = load<float>(in), inv2 = load<float>(in);  // mvScaleFactors, mvInvLevelSigma2
    const std::vector<vsg_keypoint> keys = load<vsg_keypoint>(in);
    const std::vector<uint8_t> desc = load<uint8_t>(in);
    const std::vector<float> uRight = load<float>(in);  // empty: a KeyFrame without mvuRight
    const std::vector<float> pos = load<float>(in), nrm = load<float>(in), dmin = load<float>(in), dmax = load<float>(in);
    const std::vector<uint8_t> mdesc = load<uint8_t>(in), skip = load<uint8_t>(in);
    std::vector<int32_t> matched = load<int32_t>(in);  // vpMatched on entry
    if (cam.size() != 21 || head.size() != 2 || par.size() != 7 || !in) return 2;
    const int n = (int)dmin.size();
    vsg::FramePose pose;
    for (int i = 0; i < 9; ++i) pose.Rcw[i] = cam[i];
    for (int i = 0; i < 3; ++i) pose.tcw[i] = cam[9 + i], pose.Ow[i] = cam[12 + i];
    pose.fx = cam[15], pose.fy = cam[16], pose.cx = cam[17], pose.cy = cam[18], pose.mbf = cam[19];
    pose.log_scale_factor = cam[20], pose.n_levels = head[0];

    vsg::ResidentFrame KF((int)keys.size() + 1);
    KF.Upload(keys.data(), desc.data(), uRight.empty() ? nullptr : uRight.data(), (int)keys.size(), -1, par[0], par[1],
              par[2], par[3]);
    // the map lives in slots 2 i + 1 of a store twice its size
    vsg::ResidentMapPoints mp(2 * n + 1);
    std::vector<int32_t> slots(n);
    for (int i = 0; i < n; ++i) slots[i] = 2 * i + 1;
    mp.update(slots, pos.data(), nrm.data(), dmin.data(), dmax.data(), mdesc.data(), nullptr);

    vsg::ResidentMatcher matcher(0.9f, true);
    const uint8_t *sk = skip.empty() ? nullptr : skip.data();
    std::vector<int32_t> bestIdx, bestDist, bestIdx3, bestDist3;
    vsg::ResidentMatcher::IntoKeyFrameProjection fp, fp3, sp;
    const int nFused = matcher.Fuse(KF, mp, slots, sk, pose, par[4], sf, inv2, bestIdx, bestDist, &fp);
    const int nFused3 = matcher.Fuse(KF, mp, slots, sk, pose, par[5], sf, bestIdx3, bestDist3, &fp3);
    const int nMatches = matcher.SearchByProjection(KF, mp, slots, sk, pose, head[1], par[6], sf, matched, &sp);
    std::ofstream out(argv[2], std::ios::binary);
    dump(out, std::vector<int32_t>{nFused, nFused3, nMatches, KF.N()});
    dump(out, bestIdx), dump(out, bestDist), dump(out, fp.projected), dump(out, fp.u), dump(out, fp.v), dump(out, fp.ur);
    dump(out, fp.level), dump(out, bestIdx3), dump(out, bestDist3), dump(out, fp3.projected), dump(out, fp3.level);
    dump(out, matched), dump(out, sp.projected), dump(out, sp.u), dump(out, sp.v), dump(out, sp.level);
    printf("OK %d %d %d\n", nFused, nFused3, nMatches);
    return 0;
  } catch (const std::exception &e) {
    printf("THROW %s (no CPU fallback)\n", e.what());
    return 3;
  }
}
