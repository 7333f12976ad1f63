// The motion-model and relocalisation projection searches through include/vsg_orb_adaptor.hpp from plain C++: the two
// vsg::ResidentMatcher::SearchByProjection overloads that take resident map points.  A current frame, a last frame with
// its slot list, two poses, a map and a KeyFrame's slot list come from a flat binary file written by
// tests/test_abi_projection.py; the results go to a second file the test compares with the Python binding and the
// reference.  Without a device the store throws (exit 3).
//   usage: projection_check <in.bin> <out.bin>
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

static vsg::FramePose pose_of(const std::vector<float> &cam, int n_levels) {
  vsg::FramePose p;  // Rcw[9] tcw[3] Ow[3] fx fy cx cy mbf logScaleFactor
  for (int i = 0; i < 9; ++i) p.Rcw[i] = cam[i];
  for (int i = 0; i < 3; ++i) p.tcw[i] = cam[9 + i], p.Ow[i] = cam[12 + i];
  p.fx = cam[15], p.fy = cam[16], p.cx = cam[17], p.cy = cam[18], p.mbf = cam[19];
  p.log_scale_factor = cam[20], p.n_levels = n_levels;
  return p;
}

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  try {
    vsg::ResidentMapPoints probe(16);  // no device: throws here ("no CPU fallback")
    std::ifstream in(argv[1], std::ios::binary);
    if (!in) return 2;
    const std::vector<float> cam = load<float>(in), lastCam = load<float>(in);
    const std::vector<int32_t> head = load<int32_t>(in);  // nLevels, bMono, ORBdist
    const std::vector<float> par = load<float>(in);       // bounds[4], th (last frame), th (KeyFrame), mb
    const std::vector<float> sf = load<float>(in);        // mvScaleFactors
    const std::vector<vsg_keypoint> keys = load<vsg_keypoint>(in);
    const std::vector<uint8_t> desc = load<uint8_t>(in);
    const std::vector<float> uRight = load<float>(in);    // empty: a frame without mvuRight
    const std::vector<vsg_keypoint> lastKeys = load<vsg_keypoint>(in);
    const std::vector<uint8_t> lastDesc = load<uint8_t>(in);
    const std::vector<int32_t> lastPoint = load<int32_t>(in);  // per last-frame feature: index of its map point or -1
    const std::vector<float> pos = load<float>(in), dmin = load<float>(in), dmax = load<float>(in);
    const std::vector<uint8_t> mdesc = load<uint8_t>(in), obs = load<uint8_t>(in);
    const std::vector<float> kfAngle = load<float>(in);
    const std::vector<uint8_t> skip = load<uint8_t>(in);
    if (cam.size() != 21 || lastCam.size() != 21 || head.size() != 3 || par.size() != 7 || !in) return 2;
    const int n = (int)dmin.size();
    const vsg::FramePose pose = pose_of(cam, head[0]), lastPose = pose_of(lastCam, head[0]);

    vsg::ResidentFrame F((int)keys.size() + 1), L((int)lastKeys.size() + 1);
    F.Upload(keys.data(), desc.data(), uRight.empty() ? nullptr : uRight.data(), (int)keys.size(), -1, par[0], par[1], par[2],
             par[3]);
    L.Upload(lastKeys.data(), lastDesc.data(), nullptr, (int)lastKeys.size(), -1, par[0], par[1], par[2], par[3]);
    // the map lives in slots 2 i + 1 of a store twice its size
    vsg::ResidentMapPoints mp(2 * n + 1);
    std::vector<int32_t> slots(n), lastSlots(lastPoint.size());
    for (int i = 0; i < n; ++i) slots[i] = 2 * i + 1;
    for (size_t i = 0; i < lastPoint.size(); ++i) lastSlots[i] = lastPoint[i] < 0 ? -1 : 2 * lastPoint[i] + 1;
    mp.update(slots, pos.data(), nullptr, dmin.data(), dmax.data(), mdesc.data(), obs.data());

    vsg::ResidentMatcher matcher(0.9f, true);
    std::vector<uint8_t> blocked(keys.size(), 0), occupied(keys.size(), 0);
    std::vector<int32_t> matchLast, matchKF;
    vsg::ResidentMatcher::LastFrameProjection lp;
    const int nmLast = matcher.SearchByProjection(F, L, mp, lastSlots, pose, lastPose, par[6], par[4], head[1] != 0, sf,
                                                  blocked, matchLast, &lp);
    vsg::ResidentMatcher::KeyFrameProjection kp;
    const int nmKF = matcher.SearchByProjection(F, mp, slots, kfAngle, skip.empty() ? nullptr : skip.data(), pose, par[5],
                                                head[2], sf, occupied, matchKF, &kp);
    std::ofstream out(argv[2], std::ios::binary);
    dump(out, std::vector<int32_t>{nmLast, lp.direction, nmKF, F.N()});
    dump(out, matchLast), dump(out, blocked), dump(out, lp.projected), dump(out, lp.u), dump(out, lp.v), dump(out, lp.ur);
    dump(out, matchKF), dump(out, occupied), dump(out, kp.projected), dump(out, kp.u), dump(out, kp.v), dump(out, kp.level);
    printf("OK %d %d %d\n", nmLast, lp.direction, nmKF);
    return 0;
  } catch (const std::exception &e) {
    printf("THROW %s (no CPU fallback)\n", e.what());
    return 3;
  }
}
