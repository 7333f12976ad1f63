// vsg_fv.h -- a FeatureVector (DBoW2 std::map<NodeId, std::vector<unsigned>>, Frame::mFeatVec) given by the caller as host
// arrays, for the vocabulary-node searches of vsg_match.hip: the check every entry point runs before it touches a device,
// the merge-join of two of them, and the check of the triangulation search's predicate-bit layout against the joined nodes.
// Host only and free of HIP: compiled into the library and, by tests/_fvcore, into a CPU test core and a sanitized program.
// The kernels index descriptors, flags and keypoints with idx and the bit array with pair_off: what these functions accept
// is all that reaches a device.  NOT checked: a feature listed under two nodes.  The reference's map cannot hold one, the
// kernels rely on it (a node's block is the only writer of its features' matches) and it stays the caller's contract: a
// violation gives a wrong answer, never an access outside an array.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace vsg {

// CSR view: node ids ascending, off[nodes + 1], idx[off[nodes]] feature indices
struct FvView {
  const int32_t *node_id, *off, *idx;
  int nodes;
};

// the feature ranges [a_begin, a_end) of idx of A and [b_begin, b_end) of idx of B of one vocabulary node both sides have
struct NodePair {
  int a_begin, a_end, b_begin, b_end;
};

// Is v the FeatureVector of a frame of n features?  nodes == 0 is valid whatever the pointers are (std::vector::data() of an
// empty vector) and nothing is dereferenced.  Otherwise: three arrays, offsets that start at 0 and never descend, every
// listed feature inside [0, n), and node ids STRICTLY ascending -- join_nodes bisects them, and the kernels rely on a node
// id naming one node.
inline bool fv_check(const FvView &v, int n) {
  if (v.nodes == 0) return true;
  if (v.nodes < 0 || n < 0 || !v.node_id || !v.off || !v.idx || v.off[0] != 0) return false;
  for (int k = 0; k < v.nodes; k++)
    if (v.off[k + 1] < v.off[k] || (k > 0 && v.node_id[k] <= v.node_id[k - 1])) return false;
  for (int k = 0, e = v.off[v.nodes]; k < e; k++)
    if (v.idx[k] < 0 || v.idx[k] >= n) return false;
  return true;
}

// merge-join of two FeatureVectors (ORBmatcher.cc:247-405 loop skeleton incl. lower_bound jumps)
inline void join_nodes(const int *idA, const int *offA, int nA, const int *idB, const int *offB, int nB,
                       std::vector<NodePair> &out) {
  int i = 0, j = 0;
  while (i != nA && j != nB) {
    if (idA[i] == idB[j]) {
      out.push_back({offA[i], offA[i + 1], offB[j], offB[j + 1]});
      i++, j++;
    } else if (idA[i] < idB[j]) {
      i = (int)(std::lower_bound(idA, idA + nA, idB[j]) - idA);
    } else {
      j = (int)(std::lower_bound(idB, idB + nB, idA[i]) - idB);
    }
  }
}

// The predicate bits of SearchForTriangulation: the kernel reads bit pair_off[s] + i * nb(s) + j of shared node s (in join
// order) for i < na(s), j < nb(s).  True when the first offset is not negative and every node's range holds na(s) * nb(s)
// bits (in 64-bit arithmetic: a node whose bit count does not fit the int32 offsets is refused): then every bit the kernel
// can read lies in the words [0, (pair_off[pairs.size()] + 31) / 32).  Without a shared node nothing is read.
inline bool pair_bits_check(const std::vector<NodePair> &pairs, const int32_t *pair_off) {
  if (pairs.empty()) return true;
  if (!pair_off || pair_off[0] < 0) return false;
  for (size_t s = 0; s < pairs.size(); s++) {
    const int64_t na = pairs[s].a_end - pairs[s].a_begin, nb = pairs[s].b_end - pairs[s].b_begin;
    if ((int64_t)pair_off[s + 1] - (int64_t)pair_off[s] < na * nb) return false;
  }
  return true;
}

}  // namespace vsg
