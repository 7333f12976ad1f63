// Stand-alone driver of the host core (epipolarcore.cpp: vsg::epipolar_reason_pair) for tests/test_sanitizers_epipolar.py,
// built with AddressSanitizer + UndefinedBehaviorSanitizer linked in.
//   epipolar_sanitized IN OUT
// IN holds records [int32 n, nlevels, only_stereo, coarse | x1 y1 ur1 x2 y2 ur2 (n floats each) | octave2 n (i32) | F12 9 |
// ep 2 | scale_factors2 nlevels | level_sigma2_2 nlevels] until its end; OUT gets the n reason codes of every record.  Every
// array is a heap block of exactly its size, so a step past an end is reported.
#include <cstdint>
#include <cstdio>
#include <vector>

extern "C" void ec_pair_reasons(int n, const float *x1, const float *y1, const float *ur1, const float *x2, const float *y2,
                                const float *ur2, const int32_t *octave2, const float *F12, const float *ep,
                                const float *scale_factors2, const float *level_sigma2_2, int only_stereo, int coarse,
                                uint8_t *reason);

template <class T>
static bool get(FILE *f, std::vector<T> &a) {
  return a.empty() || fread(a.data(), sizeof(T), a.size(), f) == a.size();
}

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int32_t head[4];
  while (fread(head, sizeof(head), 1, in) == 1) {
    if (head[0] < 0 || head[1] < 1 || head[1] > 16) return 3;
    const size_t n = (size_t)head[0], nl = (size_t)head[1];
    std::vector<float> v[6], F12(9), ep(2), sf(nl), s2(nl);
    for (auto &a : v) a.resize(n);
    std::vector<int32_t> oct(n);
    std::vector<uint8_t> reason(n);
    for (auto &a : v)
      if (!get(in, a)) return 3;
    if (!get(in, oct) || !get(in, F12) || !get(in, ep) || !get(in, sf) || !get(in, s2)) return 3;
    for (int32_t o : oct)
      if (o < 0 || o >= head[1]) return 3;
    ec_pair_reasons(head[0], v[0].data(), v[1].data(), v[2].data(), v[3].data(), v[4].data(), v[5].data(), oct.data(), F12.data(),
                    ep.data(), sf.data(), s2.data(), head[2], head[3], reason.data());
    if (n && fwrite(reason.data(), 1, n, out) != n) return 4;
  }
  return fclose(out) == 0 && fclose(in) == 0 ? 0 : 4;
}
