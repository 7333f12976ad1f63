// Tracking's two per-frame steps on resident data through include/vsg_orb_adaptor.hpp from plain C++: the two frames, the
// map points, the slots and the poses come from a flat binary file written by tests/test_adaptor_track.py;
// vsg::ResidentFrame::TrackWithMotionModel runs, its slots go into vsg::ResidentFrame::TrackLocalMap, and both results go
// to a second file the test compares with the C ABI's through ctypes byte for byte.
//   usage: track_check <in.bin> <out.bin>
#include <cstdio>
#include <cstring>
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
static void put(std::ofstream &o, const std::vector<T> &v) {
  o.write((const char *)v.data(), sizeof(T) * v.size());
}

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  try {
    std::ifstream in(argv[1], std::ios::binary);
    if (!in) return 2;
    // head: capacity of the store, mono, check orientation, only tracking, drop outliers
    const std::vector<int32_t> head = load<int32_t>(in);
    // scal: mb, th of the motion-model search, th of the local search, nnratio
    const std::vector<float> scal = load<float>(in);
    const std::vector<uint8_t> curKeys = load<uint8_t>(in), curDesc = load<uint8_t>(in);
    const std::vector<float> uRight = load<float>(in);
    const std::vector<uint8_t> lastKeys = load<uint8_t>(in), lastDesc = load<uint8_t>(in);
    const std::vector<int32_t> lastSlots = load<int32_t>(in);
    const std::vector<float> pos = load<float>(in), normal = load<float>(in), minDist = load<float>(in),
                             maxDist = load<float>(in);
    const std::vector<uint8_t> desc = load<uint8_t>(in), observed = load<uint8_t>(in);
    const std::vector<uint8_t> curPose = load<uint8_t>(in), lastPose = load<uint8_t>(in);
    const std::vector<float> tcw = load<float>(in), scale = load<float>(in), sigma = load<float>(in);
    const std::vector<int32_t> local = load<int32_t>(in);
    const std::vector<uint8_t> skip = load<uint8_t>(in);
    if (!in || head.size() != 5 || scal.size() != 4 || tcw.size() != 7 || curPose.size() != sizeof(vsg_frame_pose) ||
        lastPose.size() != sizeof(vsg_frame_pose) || skip.size() != local.size())
      return 2;
    const int n = (int)(curKeys.size() / sizeof(vsg_keypoint)), nl = (int)(lastKeys.size() / sizeof(vsg_keypoint));
    vsg::ResidentFrame F(n + 1), L(nl + 1);
    F.Upload((const vsg_keypoint *)curKeys.data(), curDesc.data(), uRight.empty() ? nullptr : uRight.data(), n, -1, 0.0f, 0.0f,
             640.0f, 480.0f);
    L.Upload((const vsg_keypoint *)lastKeys.data(), lastDesc.data(), nullptr, nl, -1, 0.0f, 0.0f, 640.0f, 480.0f);
    vsg::ResidentMapPoints mp(head[0]);
    std::vector<int32_t> all(head[0]);
    for (int i = 0; i < head[0]; ++i) all[i] = i;
    mp.update(all, pos.data(), normal.data(), minDist.data(), maxDist.data(), desc.data(), observed.data());
    vsg_frame_pose cp, lp;
    memcpy(&cp, curPose.data(), sizeof(cp)), memcpy(&lp, lastPose.data(), sizeof(lp));
    vsg_pose_se3 Tcw;
    for (int k = 0; k < 4; ++k) Tcw.q[k] = tcw[k];
    for (int k = 0; k < 3; ++k) Tcw.t[k] = tcw[4 + k];

    std::vector<uint8_t> outlierM(n, 7);  // mvbOutlier's storage: entries of unmatched features keep the 7
    std::vector<float> chi2M(n, -1.0f);
    vsg::ResidentFrame::TrackMotionResult m;
    const int retM = F.TrackWithMotionModel(L, mp, lastSlots, cp, lp, scal[0], head[1] != 0, scal[1], scale, head[2] != 0, Tcw,
                                            sigma, outlierM, m, false, &chi2M);
    std::vector<uint8_t> outlierL(n, 7);
    std::vector<float> chi2L(n, -1.0f);
    vsg::ResidentFrame::TrackLocalResult t;
    const int retL = F.TrackLocalMap(mp, (int)local.size(), local.data(), skip.data(), cp, scal[2], scal[3], false, 0.0f, scale,
                                     m.featSlots, Tcw, sigma, head[3] != 0, head[4] != 0, outlierL, t, false, &chi2L);

    std::ofstream o(argv[2], std::ios::binary);
    const int32_t hm[12] = {retM, m.nSearch, m.wide, m.nMatchesSearched, m.optimized, m.nMatches, m.nMatchesMap, m.direction,
                            m.pose.nInitialCorrespondences, m.pose.nBad, m.pose.roundsRun, m.pose.held};
    o.write((const char *)hm, sizeof(hm));
    put(o, m.featSlots), put(o, m.trainMatch), put(o, outlierM), put(o, chi2M);
    o.write((const char *)m.pose.qd, 32), o.write((const char *)m.pose.td, 24);
    const int32_t hl[9] = {retL, t.nToMatch, t.nMatchesSearched, t.nMatchesInliers, t.walkRounds,
                           t.pose.nInitialCorrespondences, t.pose.nBad, t.pose.roundsRun, t.pose.held};
    o.write((const char *)hl, sizeof(hl));
    put(o, t.featSlots), put(o, t.trainMatch), put(o, outlierL), put(o, chi2L);
    put(o, t.inView), put(o, t.projX), put(o, t.projY);
    o.write((const char *)t.pose.qd, 32), o.write((const char *)t.pose.td, 24);
    return o ? 0 : 2;
  } catch (const std::exception &e) {
    fprintf(stderr, "track_check: %s\n", e.what());
    return 3;
  }
}
