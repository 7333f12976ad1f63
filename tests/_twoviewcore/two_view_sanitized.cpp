// Stand-alone driver of the host core (twoviewcore.cpp: the argument check and vsg::two_view::reconstruct_host) for
// tests/test_sanitizers_two_view.py, built with AddressSanitizer + UndefinedBehaviorSanitizer linked in.
//   two_view_sanitized IN OUT
// IN holds records until its end:
//   int32 n1, n2, n_iter, two_threads, want_optional | float K[9] | vsg_two_view_params | xy1 2 n1, xy2 2 n2 (f32) |
//   matches12 n1 (i32) | sets 8 n_iter (i32)
// OUT gets per record: int32 N (the argument check: the number of matches, -1 refused), and when N >= 0:
// vsg_two_view_result, triangulated n1, x3d 3 n1 (both start as 0xAA / a sentinel float), and with want_optional inlier_h N,
// inlier_f N, score_h n_iter, score_f n_iter.  Every array is a heap block of exactly its size, so a step past an end is
// reported; a record the check refuses never reaches the routine.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/vsg_orb.h"

extern "C" {
int tv_args_ok(const float *xy1, int n1, const float *xy2, int n2, const int32_t *matches12, const float *K,
               const vsg_two_view_params *params, int n_iter, const int32_t *sets);
void tv_reconstruct(const float *xy1, int n1, const float *xy2, int n2, const int32_t *matches12, const float *K,
                    const vsg_two_view_params *params, int n_iter, const int32_t *sets, int two_threads, vsg_two_view_result *res,
                    uint8_t *triangulated, float *x3d, uint8_t *inlier_h, uint8_t *inlier_f, float *score_h, float *score_f);
}

template <class T>
static bool get(FILE *f, std::vector<T> &a) {
  return a.empty() || fread(a.data(), sizeof(T), a.size(), f) == a.size();
}
template <class T>
static bool put(FILE *f, const std::vector<T> &a) {
  return a.empty() || fwrite(a.data(), sizeof(T), a.size(), f) == a.size();
}

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int32_t head[5];
  while (fread(head, sizeof(head), 1, in) == 1) {
    for (int k = 0; k < 3; k++)
      if (head[k] < 0 || head[k] > (1 << 20)) return 3;  // sizes of the record itself
    const size_t n1 = (size_t)head[0], n2 = (size_t)head[1], ni = (size_t)head[2];
    float K[9];
    vsg_two_view_params P;
    if (fread(K, sizeof K, 1, in) != 1 || fread(&P, sizeof P, 1, in) != 1) return 3;
    std::vector<float> xy1(2 * n1), xy2(2 * n2);
    std::vector<int32_t> m12(n1), sets(8 * ni);
    if (!get(in, xy1) || !get(in, xy2) || !get(in, m12) || !get(in, sets)) return 3;
    const int32_t N = tv_args_ok(xy1.data(), head[0], xy2.data(), head[1], m12.data(), K, &P, head[2], sets.data());
    if (fwrite(&N, 4, 1, out) != 1) return 4;
    if (N < 0) continue;
    const bool opt = head[4] != 0;
    vsg_two_view_result res;
    std::vector<uint8_t> tri(n1, 0xAA), in_h(opt ? (size_t)N : 0), in_f(opt ? (size_t)N : 0);
    std::vector<float> x3d(3 * n1, -12345.0f), sc_h(opt ? ni : 0), sc_f(opt ? ni : 0);
    tv_reconstruct(xy1.data(), head[0], xy2.data(), head[1], m12.data(), K, &P, head[2], sets.data(), head[3], &res, tri.data(),
                   x3d.data(), opt ? in_h.data() : nullptr, opt ? in_f.data() : nullptr, opt ? sc_h.data() : nullptr,
                   opt ? sc_f.data() : nullptr);
    if (fwrite(&res, sizeof res, 1, out) != 1 || !put(out, tri) || !put(out, x3d) || !put(out, in_h) || !put(out, in_f) ||
        !put(out, sc_h) || !put(out, sc_f))
      return 4;
  }
  return fclose(out) == 0 && fclose(in) == 0 ? 0 : 4;
}
