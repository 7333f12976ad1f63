// Host build of the FeatureVector argument of the vocabulary-node searches (visual_sgraphs_amd/csrc/vsg_fv.h), for
// tests/test_fv_args.py and the sanitized program: the same source the library compiles.
#include "vsg_fv.h"

extern "C" {

int fc_fv_check(const int32_t *node_id, const int32_t *off, const int32_t *idx, int nodes, int n) {
  return vsg::fv_check(vsg::FvView{node_id, off, idx, nodes}, n);
}

// vsg::join_nodes; pairs gets {a_begin, a_end, b_begin, b_end} per shared node in join order (at most cap of them are
// written), the return value is their number
int fc_join_nodes(const int32_t *idA, const int32_t *offA, int nA, const int32_t *idB, const int32_t *offB, int nB,
                  int32_t *pairs, int cap) {
  std::vector<vsg::NodePair> out;
  vsg::join_nodes(idA, offA, nA, idB, offB, nB, out);
  for (size_t s = 0; s < out.size() && (int)s < cap; s++)
    pairs[4 * s] = out[s].a_begin, pairs[4 * s + 1] = out[s].a_end, pairs[4 * s + 2] = out[s].b_begin,
              pairs[4 * s + 3] = out[s].b_end;
  return (int)out.size();
}

// vsg::pair_bits_check on npairs nodes of na[s] x nb[s] rows
int fc_pair_bits_check(const int32_t *na, const int32_t *nb, int npairs, const int32_t *pair_off) {
  std::vector<vsg::NodePair> pairs;
  for (int s = 0; s < npairs; s++) pairs.push_back({0, na[s], 0, nb[s]});
  return vsg::pair_bits_check(pairs, pair_off);
}
}
