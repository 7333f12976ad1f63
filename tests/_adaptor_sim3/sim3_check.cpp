// Sim3Solver on resident map points through include/vsg_orb_adaptor.hpp from plain C++: the two point sets, poses, octaves and
// the RANSAC samples come from a flat binary file written by tests/test_abi_sim3.py; vsg::ResidentSim3Solver runs the loop of
// LoopClosing.cc:686 (iterate(20, ...) until bConverge || bNoMore) with a random_int that replays the file's samples, and
// what the loop leaves behind goes to a second file the test compares with the host build byte for byte.
//   usage: sim3_check <in.bin> <out.bin>
#include <cstdio>
#include <fstream>

#include "vsg_orb_adaptor.hpp"

template <class T>
static std::vector<T> load(std::ifstream &f, size_t n) {
  std::vector<T> v(n);
  if (n) f.read((char *)v.data(), sizeof(T) * n);
  return v;
}

// DUtils::Random::RandomInt replaced by the draw that yields the file's samples: the position of the wanted index in
// vAvailableIndices, which is then swapped out as the solver's draw does
struct Replay {
  const std::vector<int32_t> *samples;
  int n;
  size_t pos;
  std::vector<int32_t> avail;
};
static int replay(int lo, int hi, void *ctx) {
  Replay &r = *(Replay *)ctx;
  if (r.pos % 3 == 0) {
    r.avail.resize((size_t)r.n);
    for (int i = 0; i < r.n; ++i) r.avail[(size_t)i] = i;
  }
  if (r.pos >= r.samples->size() || hi != (int)r.avail.size() - 1 || lo != 0) return -1;
  const int32_t want = (*r.samples)[r.pos++];
  for (size_t k = 0; k < r.avail.size(); ++k)
    if (r.avail[k] == want) {
      r.avail[k] = r.avail.back();
      r.avail.pop_back();
      return (int)k;
    }
  return -1;
}

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  try {
    if (vsg_device_count() <= 0) {
      printf("no HIP device: vsg::ResidentSim3Solver has no CPU fallback\n");
      return 3;
    }
    std::ifstream in(argv[1], std::ios::binary);
    if (!in) return 2;
    const std::vector<int32_t> head = load<int32_t>(in, 3);  // n, n_hyp, min_inliers
    if (!in || head[0] < 3 || head[1] < 1) return 2;
    const int n = head[0], nh = head[1], minInliers = head[2];
    vsg::FramePose pose[2];
    in.read((char *)pose, sizeof pose);
    const std::vector<float> Xw1 = load<float>(in, 3 * (size_t)n), Xw2 = load<float>(in, 3 * (size_t)n), sigma2 = load<float>(in, 8);
    const std::vector<int32_t> oct1 = load<int32_t>(in, n), oct2 = load<int32_t>(in, n), samples = load<int32_t>(in, 3 * (size_t)nh);
    if (!in) return 2;
    vsg::ResidentMapPoints mp1(n + 5), mp2(n + 9);
    std::vector<int32_t> slots1(n), slots2(n);
    std::vector<float> e1(n), e2(n);
    std::vector<size_t> indices1(n);
    for (int i = 0; i < n; ++i) {
      slots1[i] = i + 2, slots2[i] = n + 3 - i, indices1[i] = (size_t)i;
      e1[i] = vsg::Sim3MaxError(sigma2, oct1[i]), e2[i] = vsg::Sim3MaxError(sigma2, oct2[i]);
    }
    mp1.update(slots1, Xw1.data(), nullptr, nullptr, nullptr, nullptr, nullptr);
    mp2.update(slots2, Xw2.data(), nullptr, nullptr, nullptr, nullptr, nullptr);
    Replay rp{&samples, n, 0, {}};
    vsg::ResidentSim3Solver solver(mp1, mp2, slots1, slots2, e1, e2, indices1, n, pose[0], pose[1], false, replay, &rp);
    solver.SetRansacParameters(0.99, minInliers, 300);
    if (solver.maxIterations() != nh) {
      fprintf(stderr, "sim3_check: mRansacMaxIts %d, the file has %d hypotheses\n", solver.maxIterations(), nh);
      return 2;
    }
    bool bNoMore = false, bConverge = false;
    std::vector<bool> vbInliers;
    int nInliers = 0, calls = 0;
    vsg::ResidentSim3Solver::Matrix T;
    while (!bConverge && !bNoMore) {  // LoopClosing.cc:686
      T = solver.iterate(20, bNoMore, vbInliers, nInliers, bConverge);
      if (++calls > 1000) return 4;
    }
    std::ofstream o(argv[2], std::ios::binary);
    const int32_t h[3] = {calls, bConverge ? 1 : 0, bConverge ? nInliers : solver.result().n_inliers};
    o.write((const char *)h, sizeof h);
    for (int i = 0; i < n; ++i) o.put(vbInliers[(size_t)i] ? 1 : 0);
    o.write((const char *)T.data(), 64);
    const vsg::ResidentSim3Solver::Matrix R = solver.GetEstimatedRotation();
    const std::vector<float> t = solver.GetEstimatedTranslation();
    const float s = solver.GetEstimatedScale();
    o.write((const char *)R.data(), 36), o.write((const char *)t.data(), 12), o.write((const char *)&s, 4);
    if (!o) return 2;
    printf("OK %d calls, converged %d, %d inliers\n", calls, (int)bConverge, nInliers);
    return 0;
  } catch (const std::exception &e) {
    fprintf(stderr, "sim3_check: %s\n", e.what());
    return 3;
  }
}
