// Optimizer::OptimizeEssentialGraph on resident map points through include/vsg_orb_adaptor.hpp from plain C++: the store's
// positions, the Sim3 arrays, the flags, the edge list and the points come from a flat binary file written by
// tests/test_gpu_essential_graph.py; vsg::ResidentMapPoints::OptimizeEssentialGraph runs on them and its result, with the
// whole store read back, goes to a second file the test compares with the bytes of the raw call.  The edge list is also
// rebuilt with vsg::essential_graph_edges from a chain's arrays, so that the builder is compiled and run from C++.  Without a
// device the store throws (exit 3).
//   usage: eg_check <in.bin> <out.bin>
#include <cstdio>
#include <fstream>

#include "vsg_orb_adaptor.hpp"

template <class T>
static std::vector<T> load(std::ifstream &f, size_t n) {
  std::vector<T> v(n);
  if (n) f.read((char *)v.data(), sizeof(T) * n);
  return v;
}
template <class T>
static void dump(std::ofstream &f, const std::vector<T> &v) {
  if (!v.empty()) f.write((const char *)v.data(), sizeof(T) * v.size());
}

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  try {
    vsg::ResidentMapPoints probe(16);  // no device: throws here ("no CPU fallback")
    // a chain of three keyframes through the builder: 1 -> 0 and 2 -> 1 from the spanning tree, 2 -> 0 from covisibility
    const vsg::EssentialGraphEdges chain = vsg::essential_graph_edges(3, {-1, 0, 1}, {0, 0, 0, 0}, {}, {0, 1, 2, 2}, {1, 2}, {0, 1, 3, 5},
                                                                      {1, 0, 2, 1, 0}, {}, {0}, {}, {}, 2, 0);
    if (chain.i != std::vector<int32_t>{1, 2, 2} || chain.j != std::vector<int32_t>{0, 1, 0}) return 4;
    std::ifstream in(argv[1], std::ios::binary);
    if (!in) return 2;
    const std::vector<int32_t> head = load<int32_t>(in, 6);  // capacity, keyframes, edges, points, fix_scale, iterations
    if (!in || head[0] < 0 || head[1] < 0 || head[2] < 0 || head[3] < 0) return 2;
    const size_t cap = (size_t)head[0], K = (size_t)head[1], E = (size_t)head[2], P = (size_t)head[3];
    const std::vector<float> pos = load<float>(in, 3 * cap);
    const std::vector<vsg_sim3d> Scw = load<vsg_sim3d>(in, K), nonc = load<vsg_sim3d>(in, K);
    const std::vector<uint8_t> has = load<uint8_t>(in, K), fixed = load<uint8_t>(in, K);
    vsg::EssentialGraphEdges edges;
    edges.i = load<int32_t>(in, E), edges.j = load<int32_t>(in, E), edges.loop = load<uint8_t>(in, E);
    const std::vector<int32_t> slots = load<int32_t>(in, P), ref = load<int32_t>(in, P);
    if (!in) return 2;
    std::vector<int32_t> all(cap);
    for (size_t i = 0; i < cap; ++i) all[i] = (int32_t)i;
    vsg::ResidentMapPoints mp((int)cap);
    mp.update(all, pos.data(), nullptr, nullptr, nullptr, nullptr, nullptr);  // SetWorldPos
    const vsg::EssentialGraphResult r = mp.OptimizeEssentialGraph(Scw, nonc, has, fixed, edges, head[4] != 0, slots, ref, head[5]);
    std::vector<float> after(3 * cap);
    vsg::check(vsg_mappoints_read(mp.handle(), (int)cap, all.data(), after.data(), nullptr, nullptr, nullptr, nullptr, nullptr),
               "vsg_mappoints_read");
    // CorrectSim3 with identities leaves every listed position as it is
    std::vector<vsg_sim3d> id(K);
    for (auto &s : id) s = vsg_sim3d{{0, 0, 0, 1}, {0, 0, 0}, 1};
    const std::vector<float> same = mp.CorrectSim3(slots, ref, id, id);
    for (size_t i = 0; i < P; ++i)
      for (int d = 0; d < 3; ++d)
        if (same[3 * i + d] != after[3 * (size_t)slots[i] + d]) return 5;
    std::ofstream out(argv[2], std::ios::binary);
    dump(out, r.kfScw), dump(out, r.worldPos), dump(out, r.chi2), dump(out, after);
    printf("OK %d %d\n", (int)K, r.res.trials_run);
    return 0;
  } catch (const std::exception &e) {
    printf("THROW %s (no CPU fallback)\n", e.what());
    return 3;
  }
}
