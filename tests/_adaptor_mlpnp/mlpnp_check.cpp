// MLPnPsolver on a resident frame through include/vsg_orb_adaptor.hpp from plain C++: the frame's keypoints, the slots, the
// store's positions and the minimal sets come from a flat binary file written by tests/test_gpu_adaptor_mlpnp.py;
// vsg::MLPnPsolver runs the loop of Tracking.cc:3762 (iterate(5, ...) until it returns true or bNoMore) with a random_int
// that replays the file's sets, and every call's return goes to a second file the test compares with the sequential
// restatement's sequence of returns.
//   usage: mlpnp_check <in.bin> <out.bin>
#include <cstdio>
#include <fstream>

#include "vsg_orb_adaptor.hpp"

template <class T>
static std::vector<T> load(std::ifstream &f, size_t n) {
  std::vector<T> v(n);
  if (n) f.read((char *)v.data(), sizeof(T) * n);
  return v;
}

// DUtils::Random::RandomInt replaced by the draw that yields the file's sets: the position of the wanted index in
// vAvailableIndices, which is then swapped out as the solver's draw does
struct Replay {
  const std::vector<int32_t> *sets;
  int n;
  size_t pos;
  std::vector<int32_t> avail;
};
static int replay(int lo, int hi, void *ctx) {
  Replay &r = *(Replay *)ctx;
  if (r.pos % 6 == 0) {
    r.avail.resize((size_t)r.n);
    for (int i = 0; i < r.n; ++i) r.avail[(size_t)i] = i;
  }
  if (r.pos >= r.sets->size() || hi != (int)r.avail.size() - 1 || lo != 0) return -1;
  const int32_t want = (*r.sets)[r.pos++];
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
      printf("no HIP device: vsg::MLPnPsolver has no CPU fallback\n");
      return 3;
    }
    std::ifstream in(argv[1], std::ios::binary);
    if (!in) return 2;
    const std::vector<int32_t> head = load<int32_t>(in, 4);  // n_feat, capacity, n_hyp, nlevels
    if (!in || head[0] < 1 || head[1] < 1 || head[2] < 1 || head[3] < 1) return 2;
    const int nf = head[0], cap = head[1], nh = head[2], nl = head[3];
    const std::vector<float> K4 = load<float>(in, 4), sigma2 = load<float>(in, (size_t)nl), kx = load<float>(in, (size_t)nf),
                             ky = load<float>(in, (size_t)nf);
    const std::vector<int32_t> octave = load<int32_t>(in, (size_t)nf), slots = load<int32_t>(in, (size_t)nf);
    const std::vector<float> world = load<float>(in, 3 * (size_t)cap);
    const std::vector<int32_t> sets = load<int32_t>(in, 6 * (size_t)nh);
    if (!in) return 2;
    std::vector<vsg_keypoint> keys((size_t)nf);
    for (int i = 0; i < nf; ++i) keys[(size_t)i] = vsg_keypoint{kx[(size_t)i], ky[(size_t)i], 31.0f, -1.0f, 0.0f, octave[(size_t)i], -1};
    const std::vector<uint8_t> desc(32 * (size_t)nf, 0);
    vsg::ResidentFrame F(nf + 1);
    F.Upload(keys.data(), desc.data(), nullptr, nf, -1, 0.0f, 0.0f, 640.0f, 480.0f);
    vsg::ResidentMapPoints mp(cap);
    std::vector<int32_t> all((size_t)cap);
    for (int i = 0; i < cap; ++i) all[(size_t)i] = i;
    mp.update(all, world.data(), nullptr, nullptr, nullptr, nullptr, nullptr);
    int n = 0;
    for (int32_t s : slots) n += s >= 0 ? 1 : 0;
    Replay rp{&sets, n, 0, {}};
    vsg::MLPnPsolver solver(F, mp, slots, K4.data(), sigma2, replay, &rp);
    solver.SetRansacParameters(0.99, 10, 300, 6, 0.5, 5.991);  // Tracking.cc:3736
    bool bNoMore = false, bTcw = false;
    std::vector<bool> vbInliers;
    int nInliers = 0, calls = 0;
    vsg::MLPnPsolver::Matrix Tcw;
    std::ofstream o(argv[2], std::ios::binary);
    const int32_t h0[3] = {solver.correspondences(), solver.minInliers(), solver.maxIterations()};
    o.write((const char *)h0, sizeof h0);
    while (!bNoMore && !bTcw) {  // Tracking.cc:3755-3762
      bTcw = solver.iterate(5, bNoMore, vbInliers, nInliers, Tcw);
      const int32_t h[4] = {bTcw ? 1 : 0, bNoMore ? 1 : 0, nInliers, solver.iterations()};
      o.write((const char *)h, sizeof h);
      if (++calls > 1000) return 4;
    }
    const int32_t end[2] = {-1, (int32_t)vbInliers.size()};
    o.write((const char *)end, sizeof end);
    for (size_t i = 0; i < vbInliers.size(); ++i) o.put(vbInliers[i] ? 1 : 0);
    o.write((const char *)Tcw.data(), 64);
    if (!o) return 2;
    printf("OK %d calls, found %d, no more %d, %d inliers\n", calls, (int)bTcw, (int)bNoMore, nInliers);
    return 0;
  } catch (const std::exception &e) {
    fprintf(stderr, "mlpnp_check: %s\n", e.what());
    return 3;
  }
}
