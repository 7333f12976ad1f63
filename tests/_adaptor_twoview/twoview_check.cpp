// TwoViewReconstruction through include/vsg_orb_adaptor.hpp from plain C++: two frames of undistorted keypoints, vMatches12, K,
// the parameters and the minimal sets come from a flat binary file written by tests/test_gpu_adaptor_twoview.py;
// vsg::ResidentTwoViewReconstruction runs Reconstruct on two resident frames and again on the keypoint vectors, with a
// random_int that replays the file's sets, and what both calls leave behind goes to a second file the test compares with the
// host build byte for byte.
//   usage: twoview_check <in.bin> <out.bin>
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
// vAvailableIndices, which is then swapped out as the reference's draw does
struct Replay {
  const std::vector<int32_t> *sets;
  int n;
  size_t pos;
  std::vector<int32_t> avail;
};
static int replay(int lo, int hi, void *ctx) {
  Replay &r = *(Replay *)ctx;
  if (r.pos % 8 == 0) {
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
      printf("no HIP device: vsg::ResidentTwoViewReconstruction has no CPU fallback\n");
      return 3;
    }
    std::ifstream in(argv[1], std::ios::binary);
    if (!in) return 2;
    const std::vector<int32_t> head = load<int32_t>(in, 4);  // n1, n2, n_iter, min_triangulated
    const std::vector<float> fl = load<float>(in, 11);       // K[9], sigma, rh_threshold
    if (!in || head[0] < 8 || head[1] < 1 || head[2] < 1) return 2;
    const int n1 = head[0], n2 = head[1], ni = head[2];
    const std::vector<float> xy1 = load<float>(in, 2 * (size_t)n1), xy2 = load<float>(in, 2 * (size_t)n2);
    const std::vector<int32_t> m12 = load<int32_t>(in, n1), sets = load<int32_t>(in, 8 * (size_t)ni);
    const std::vector<float> p3d_in = load<float>(in, 3 * (size_t)n1);  // what vP3D holds before the call
    if (!in) return 2;
    std::vector<vsg_keypoint> k1(n1), k2(n2);
    for (int i = 0; i < n1; ++i) k1[i] = vsg_keypoint{xy1[2 * i], xy1[2 * i + 1], 31.f, 0.f, 0.f, 0, -1};
    for (int i = 0; i < n2; ++i) k2[i] = vsg_keypoint{xy2[2 * i], xy2[2 * i + 1], 31.f, 0.f, 0.f, 0, -1};
    const std::vector<uint8_t> d1(32 * (size_t)n1, 0), d2(32 * (size_t)n2, 0);
    vsg::ResidentFrame F1(n1 + 3), F2(n2 + 7);
    F1.Upload(k1.data(), d1.data(), nullptr, n1, -1, 0.f, 0.f, 640.f, 480.f);
    F2.Upload(k2.data(), d2.data(), nullptr, n2, -1, 0.f, 0.f, 640.f, 480.f);
    int N = 0;
    for (int m : m12) N += m >= 0 ? 1 : 0;
    std::vector<int> vMatches12(m12.begin(), m12.end());
    std::ofstream o(argv[2], std::ios::binary);
    int oks = 0;
    for (int form = 0; form < 2; ++form) {
      Replay rp{&sets, N, 0, {}};
      vsg::ResidentTwoViewReconstruction tvr(fl.data(), fl[9], ni, 0, replay, &rp);
      tvr.params().rh_threshold = fl[10], tvr.params().min_triangulated = head[3];
      float R21[9] = {0}, t21[3] = {0};
      std::vector<float> vP3D = p3d_in;
      std::vector<bool> vbTriangulated;
      const bool ok = form == 0 ? tvr.Reconstruct(F1, F2, vMatches12, R21, t21, vP3D, vbTriangulated)
                                : tvr.Reconstruct(k1, k2, vMatches12, R21, t21, vP3D, vbTriangulated);
      if (tvr.sets() != sets) {
        fprintf(stderr, "twoview_check: the replayed draw differs from the file's sets\n");
        return 2;
      }
      oks += ok ? 1 : 0;
      const int32_t h[2] = {ok ? 1 : 0, (int32_t)vbTriangulated.size()};
      o.write((const char *)h, sizeof h);
      o.write((const char *)&tvr.result(), sizeof(vsg_two_view_result));
      o.write((const char *)R21, sizeof R21), o.write((const char *)t21, sizeof t21);
      for (size_t i = 0; i < vbTriangulated.size(); ++i) o.put(vbTriangulated[i] ? 1 : 0);
      o.write((const char *)vP3D.data(), sizeof(float) * vP3D.size());
    }
    if (!o) return 2;
    printf("OK %d of 2 calls succeeded\n", oks);
    return 0;
  } catch (const std::exception &e) {
    fprintf(stderr, "twoview_check: %s\n", e.what());
    return 3;
  }
}
