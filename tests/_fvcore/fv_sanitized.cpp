// Stand-alone driver of the host core (fvcore.cpp: vsg::fv_check, join_nodes, pair_bits_check of csrc/vsg_fv.h) for
// tests/test_sanitizers_fv.py, built with AddressSanitizer + UndefinedBehaviorSanitizer linked in.
//   fv_sanitized IN OUT
// IN holds records of int32 until its end, each behind a head of five {kind, a, b, c, d}:
//   kind 0  fv_check:        nodes = a, n = b, node_id[a] off[a + 1] idx[c]; d != 0: the three arrays are NULL   -> 1 result
//   kind 1  join_nodes:      idA[a] offA[a + 1] idB[b] offB[b + 1]                       -> count, then 4 ints per shared node
//   kind 2  pair_bits_check: na[a] nb[a] pair_off[a + 1]                                                     -> 1 result
// OUT gets the results as int32.  Every array is a heap block of exactly its size, so a step past an end is reported.
#include <cstdint>
#include <cstdio>
#include <vector>

extern "C" int fc_fv_check(const int32_t *node_id, const int32_t *off, const int32_t *idx, int nodes, int n);
extern "C" int fc_join_nodes(const int32_t *idA, const int32_t *offA, int nA, const int32_t *idB, const int32_t *offB, int nB,
                             int32_t *pairs, int cap);
extern "C" int fc_pair_bits_check(const int32_t *na, const int32_t *nb, int npairs, const int32_t *pair_off);

typedef std::vector<int32_t> Ints;
static bool get(FILE *f, Ints &a, size_t n) {
  a.resize(n);
  a.shrink_to_fit();
  return n == 0 || fread(a.data(), 4, n, f) == n;
}
static bool put(FILE *f, const Ints &a) { return a.empty() || fwrite(a.data(), 4, a.size(), f) == a.size(); }

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int32_t head[5];
  while (fread(head, sizeof(head), 1, in) == 1) {
    if (head[1] < 0 || head[2] < 0 || head[3] < 0) return 3;
    const size_t a = (size_t)head[1], b = (size_t)head[2], c = (size_t)head[3];
    Ints v[4], res;
    if (head[0] == 0) {
      if (!get(in, v[0], a) || !get(in, v[1], a + 1) || !get(in, v[2], c)) return 3;
      res.push_back(head[4] ? fc_fv_check(nullptr, nullptr, nullptr, head[1], head[2])
                            : fc_fv_check(v[0].data(), v[1].data(), v[2].data(), head[1], head[2]));
    } else if (head[0] == 1) {
      if (!get(in, v[0], a) || !get(in, v[1], a + 1) || !get(in, v[2], b) || !get(in, v[3], b + 1)) return 3;
      const size_t cap = a < b ? a : b;  // a node is shared at most once
      Ints pairs(4 * cap);
      const int count = fc_join_nodes(v[0].data(), v[1].data(), head[1], v[2].data(), v[3].data(), head[2], pairs.data(), (int)cap);
      if (count < 0 || (size_t)count > cap) return 5;
      res.push_back(count);
      res.insert(res.end(), pairs.begin(), pairs.begin() + 4 * count);
    } else if (head[0] == 2) {
      if (!get(in, v[0], a) || !get(in, v[1], a) || !get(in, v[2], a + 1)) return 3;
      res.push_back(fc_pair_bits_check(v[0].data(), v[1].data(), head[1], v[2].data()));
    } else {
      return 3;
    }
    if (!put(out, res)) return 4;
  }
  return fclose(out) == 0 && fclose(in) == 0 ? 0 : 4;
}
