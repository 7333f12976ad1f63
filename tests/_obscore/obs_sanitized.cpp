// Stand-alone driver of the host core (obscore.cpp: vsg::obs_check of csrc/vsg_obs_args.h and
// vsg::update_normal_and_depth of csrc/vsg_observations.h) for tests/test_sanitizers_observations.py, built with
// AddressSanitizer + UndefinedBehaviorSanitizer linked in.
//   obs_sanitized IN OUT
// IN holds records of int32 until its end, each behind a head of eight {kind, n, total, n_kf, capacity, nlevels, flags, -}:
//   kind 0  obs_check: slots[n] off[n + 1] kf[total] idx[total] bad[total] ref_pos[n] kf_n[n_kf] kf_oct[sum kf_n]
//           flags & 1: bad is NULL (its block is still read from IN); flags & 2: every array is NULL (n == 0)
//           -> rc, then good[n] when rc is not VSG_ERR_INVALID
//   kind 1  update_normal_and_depth: off[n + 1] kf[total] ref_pos[n] ref_level[n], then as float32 P[3 n] Ow[3 n_kf]
//           scale_factors[nlevels]                              -> normal[3 n] min_dist[n] max_dist[n] as float32 bits
// OUT gets the results as int32.  Every array is a heap block of exactly its size, so a step past an end is reported.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

extern "C" void oc_update_normal_and_depth(int n, const float *P, const int32_t *off, const int32_t *kf, const float *Ow,
                                           const int32_t *ref_pos, const int32_t *ref_level, const float *scale_factors,
                                           int nlevels, float *normal, float *min_dist, float *max_dist);
extern "C" int oc_obs_check(int n, const int32_t *slots, const int32_t *off, const int32_t *kf, const int32_t *idx,
                            const uint8_t *bad, const int32_t *ref_pos, int n_kf, const int32_t *kf_n, const int32_t *kf_oct,
                            int capacity, int nlevels, int32_t *good);

typedef std::vector<int32_t> Ints;
typedef std::vector<float> Floats;
template <class V>
static bool get(FILE *f, V &a, size_t n) {
  a.resize(n);
  a.shrink_to_fit();
  return n == 0 || fread(a.data(), 4, n, f) == n;
}
static bool put(FILE *f, const void *p, size_t n) { return n == 0 || fwrite(p, 4, n, f) == n; }

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int32_t head[8];
  while (fread(head, sizeof(head), 1, in) == 1) {
    if (head[1] < 0 || head[2] < 0 || head[3] < 0) return 3;
    const size_t n = (size_t)head[1], total = (size_t)head[2], n_kf = (size_t)head[3];
    if (head[0] == 0) {
      Ints slots, off, kf, idx, bad32, ref, kf_n, oct;
      if (!get(in, slots, n) || !get(in, off, n + 1) || !get(in, kf, total) || !get(in, idx, total) ||
          !get(in, bad32, total) || !get(in, ref, n) || !get(in, kf_n, n_kf))
        return 3;
      size_t feats = 0;
      for (int32_t v : kf_n) feats += (size_t)v;
      if (!get(in, oct, feats)) return 3;
      std::vector<uint8_t> bad(bad32.begin(), bad32.end());
      bad.shrink_to_fit();
      Ints good(n, -1);
      good.shrink_to_fit();
      const bool null_all = head[6] & 2;
      const int rc = null_all ? oc_obs_check(head[1], nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, head[3], nullptr,
                                             nullptr, head[4], head[5], nullptr)
                              : oc_obs_check(head[1], slots.data(), off.data(), kf.data(), idx.data(),
                                             head[6] & 1 ? nullptr : bad.data(), ref.data(), head[3], kf_n.data(), oct.data(),
                                             head[4], head[5], good.data());
      if (!put(out, &rc, 1)) return 4;
      if (rc != -6 && !put(out, good.data(), n)) return 4;
    } else if (head[0] == 1) {
      if (head[5] < 1) return 3;
      Ints off, kf, ref, lvl;
      Floats P, Ow, sf;
      if (!get(in, off, n + 1) || !get(in, kf, total) || !get(in, ref, n) || !get(in, lvl, n) || !get(in, P, 3 * n) ||
          !get(in, Ow, 3 * n_kf) || !get(in, sf, (size_t)head[5]))
        return 3;
      Floats nrm(3 * n, 0.0f), mn(n, 0.0f), mx(n, 0.0f);
      nrm.shrink_to_fit(), mn.shrink_to_fit(), mx.shrink_to_fit();
      oc_update_normal_and_depth(head[1], P.data(), off.data(), kf.data(), Ow.data(), ref.data(), lvl.data(), sf.data(),
                                 head[5], nrm.data(), mn.data(), mx.data());
      if (!put(out, nrm.data(), 3 * n) || !put(out, mn.data(), n) || !put(out, mx.data(), n)) return 4;
    } else {
      return 3;
    }
  }
  return fclose(out) == 0 && fclose(in) == 0 ? 0 : 4;
}
