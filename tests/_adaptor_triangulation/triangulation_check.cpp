// SearchForTriangulation with the epipolar test on the device through include/vsg_orb_adaptor.hpp from plain C++: the
// vsg::ResidentMatcher::SearchForTriangulation overload that takes F12 and the epipole, against the predicate overload given
// a lambda that calls the HOST build of csrc/vsg_epipolar.h (the caller-side loop the new overload replaces).  Two frames,
// their flags and FeatureVectors, F12, ep and the level tables come from a flat binary file written by
// tests/test_abi_triangulation.py; the pairs of every leg go to a second file the test compares with the CPU oracle.
// Exit 4 when the two overloads differ; without a device the first frame throws (exit 3).
//   usage: triangulation_check <in.bin> <out.bin>
#include <cstdio>
#include <fstream>

#include "vsg_epipolar.h"
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
static vsg::FeatureVectorCSR load_fv(std::ifstream &f) {
  vsg::FeatureVectorCSR fv;
  fv.node = load<int32_t>(f), fv.off = load<int32_t>(f), fv.idx = load<int32_t>(f);
  return fv;
}

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  try {
    vsg::ResidentFrame probe(16);  // no device: throws here ("no CPU fallback")
    std::ifstream in(argv[1], std::ios::binary);
    if (!in) return 2;
    std::vector<vsg_keypoint> keys[2];
    std::vector<uint8_t> desc[2], noMp[2];
    std::vector<float> uRight[2];
    vsg::FeatureVectorCSR fv[2];
    for (int t = 0; t < 2; ++t) {
      keys[t] = load<vsg_keypoint>(in), desc[t] = load<uint8_t>(in), uRight[t] = load<float>(in);
      noMp[t] = load<uint8_t>(in), fv[t] = load_fv(in);
    }
    const std::vector<float> F12 = load<float>(in), ep = load<float>(in), sf = load<float>(in), sigma2 = load<float>(in);
    const std::vector<float> bounds = load<float>(in);
    if (F12.size() != 9 || ep.size() != 2 || sf.size() != sigma2.size() || bounds.size() != 4 || !in) return 2;
    vsg::ResidentFrame K1((int)keys[0].size() + 1), K2((int)keys[1].size() + 1);
    vsg::ResidentFrame *K[2] = {&K1, &K2};
    for (int t = 0; t < 2; ++t)
      K[t]->Upload(keys[t].data(), desc[t].data(), uRight[t].data(), (int)keys[t].size(), -1, bounds[0], bounds[1], bounds[2],
                   bounds[3]);
    std::ofstream out(argv[2], std::ios::binary);
    int total = 0;
    for (int leg = 0; leg < 8; ++leg) {  // bOnlyStereo x bCoarse x mbCheckOrientation
      const bool onlyStereo = leg & 1, coarse = (leg & 2) != 0;
      vsg::ResidentMatcher matcher(0.6f, (leg & 4) != 0);
      std::vector<std::pair<size_t, size_t>> got, want;
      const int n = matcher.SearchForTriangulation(K1, noMp[0].data(), K2, noMp[1].data(), F12.data(), ep.data(), sf, sigma2,
                                                   onlyStereo, coarse, got, &fv[0], &fv[1]);
      // what the caller did before: the predicate on the host for every pair, shipped as a bitmask
      auto pred = [&](int i1, int i2) {
        const vsg_keypoint &a = keys[0][i1], &b = keys[1][i2];
        return vsg::epipolar_reason_pair(F12.data(), ep.data(), a.x, a.y, uRight[0][i1], b.x, b.y, uRight[1][i2], sf[b.octave],
                                         sigma2[b.octave], onlyStereo, coarse) == vsg::kEpiPass;
      };
      const int m = matcher.SearchForTriangulation(K1, noMp[0].data(), fv[0], K2, noMp[1].data(), fv[1], pred, want);
      if (n != m || got != want) {
        printf("leg %d: the epipolar overload differs from the predicate overload (%d vs %d)\n", leg, n, m);
        return 4;
      }
      std::vector<int32_t> flat{n};
      for (auto &pr : got) flat.push_back((int32_t)pr.first), flat.push_back((int32_t)pr.second);
      dump(out, flat);
      total += n;
    }
    printf("OK %d\n", total);
    return 0;
  } catch (const std::exception &e) {
    printf("THROW %s (no CPU fallback)\n", e.what());
    return 3;
  }
}
