// Stand-alone driver of the host core (sim3core.cpp: the argument check and vsg::sim3::ransac_host) for
// tests/test_sanitizers_sim3.py, built with AddressSanitizer + UndefinedBehaviorSanitizer linked in.
//   sim3_sanitized IN OUT
// IN holds records until its end:
//   int32 n, n_hyp, min_inliers, fix_scale, capacity1, capacity2, early_exit, want_hyp | vsg_frame_pose kf1, kf2 |
//   slots1 n, slots2 n (i32) | Xw1 3 n, Xw2 3 n, max_err1 n, max_err2 n (f32) | samples 3 n_hyp (i32)
// OUT gets per record: int32 ok (the argument check), and when ok: inlier n, vsg_sim3_result, and with want_hyp
// hyp_inliers n_hyp, hyp_T12 16 n_hyp.  Every array is a heap block of exactly its size, so a step past an end is reported;
// a record the check refuses never reaches the solver.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/vsg_orb.h"

extern "C" {
int sc_args_ok(int n, const int32_t *slots1, const int32_t *slots2, int capacity1, int capacity2, const float *max_err1,
               const float *max_err2, int min_inliers, int n_hyp, const int32_t *samples, const uint8_t *inlier);
void sc_ransac(int n, const float *Xw1, const float *Xw2, const float *max_err1, const float *max_err2, const vsg_frame_pose *kf1,
               const vsg_frame_pose *kf2, int fix_scale, int min_inliers, int n_hyp, const int32_t *samples, int early_exit,
               uint8_t *inlier, vsg_sim3_result *res, int32_t *hyp_inliers, float *hyp_T12);
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
  int32_t head[8];
  while (fread(head, sizeof(head), 1, in) == 1) {
    if (head[0] < 0 || head[0] > (1 << 20) || head[1] < 0 || head[1] > (1 << 20)) return 3;  // sizes of the record itself
    const size_t n = (size_t)head[0], nh = (size_t)head[1];
    vsg_frame_pose kf[2];
    if (fread(kf, sizeof(kf), 1, in) != 1) return 3;
    std::vector<int32_t> slots1(n), slots2(n), samples(3 * nh), hyp_inliers(head[7] ? nh : 0);
    std::vector<float> Xw1(3 * n), Xw2(3 * n), e1(n), e2(n), hyp_T12(head[7] ? 16 * nh : 0);
    std::vector<uint8_t> inlier(n ? n : 1);
    if (!get(in, slots1) || !get(in, slots2) || !get(in, Xw1) || !get(in, Xw2) || !get(in, e1) || !get(in, e2) || !get(in, samples))
      return 3;
    const int32_t ok = sc_args_ok(head[0], slots1.data(), slots2.data(), head[4], head[5], e1.data(), e2.data(), head[2], head[1],
                                  samples.data(), inlier.data());
    if (fwrite(&ok, 4, 1, out) != 1) return 4;
    if (!ok) continue;
    vsg_sim3_result res;
    sc_ransac(head[0], Xw1.data(), Xw2.data(), e1.data(), e2.data(), &kf[0], &kf[1], head[3], head[2], head[1], samples.data(),
              head[6], inlier.data(), &res, head[7] ? hyp_inliers.data() : nullptr, head[7] ? hyp_T12.data() : nullptr);
    inlier.resize(n);
    if (!put(out, inlier) || fwrite(&res, sizeof res, 1, out) != 1 || !put(out, hyp_inliers) || !put(out, hyp_T12)) return 4;
  }
  return fclose(out) == 0 && fclose(in) == 0 ? 0 : 4;
}
