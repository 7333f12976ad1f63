// Stand-alone driver of the host core (mlpnpcore.cpp: the argument check and vsg::mlpnp::ransac_host) for
// tests/test_sanitizers_mlpnp.py, built with AddressSanitizer + UndefinedBehaviorSanitizer linked in.
//   mlpnp_sanitized IN OUT
// IN holds records until its end:
//   int32 n_feat, n_hyp, capacity, nlevels, min_inliers, max_its, first, n_iterations, want_hyp | float th2, cam[4] |
//   slots n_feat, octave n_feat (i32) | world_pos 3 capacity, kx n_feat, ky n_feat, level_sigma2 nlevels (f32) |
//   sets 6 n_hyp (i32)
// OUT gets per record: int32 ok (the argument check), and when ok: inlier n_feat, vsg_mlpnp_result, and with want_hyp
// hyp_inliers n_hyp, hyp_T 12 n_hyp.  Every array is a heap block of exactly its size, so a step past an end is reported;
// a record the check refuses never reaches the solver.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/vsg_orb.h"

extern "C" {
int mc_args_ok(int n_feat, const int32_t *slots, int capacity, const float *level_sigma2, int nlevels, const int32_t *octave, float th2,
               int min_inliers, int max_its, int first, int n_iterations, int n_hyp, const int32_t *sets, const uint8_t *inlier,
               const vsg_mlpnp_result *res, int *n);
void mc_ransac(int n_feat, const int32_t *slots, const float *world_pos, const float *kx, const float *ky, const int32_t *octave,
               const float *cam, const float *level_sigma2, float th2, int min_inliers, int max_its, int first, int n_iterations,
               int n_hyp, const int32_t *sets, int n, uint8_t *inlier, vsg_mlpnp_result *res, int32_t *hyp_inliers, double *hyp_T);
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
  int32_t head[9];
  while (fread(head, sizeof(head), 1, in) == 1) {
    for (int k = 0; k < 4; k++)
      if (head[k] < 0 || head[k] > (1 << 20)) return 3;  // sizes of the record itself
    const size_t nf = (size_t)head[0], nh = (size_t)head[1], cap = (size_t)head[2], nl = (size_t)head[3];
    float fl[5];
    if (fread(fl, sizeof(fl), 1, in) != 1) return 3;
    std::vector<int32_t> slots(nf), octave(nf), sets(6 * nh), hyp_inliers(head[8] ? nh : 0);
    std::vector<float> world(3 * cap), kx(nf), ky(nf), sigma2(nl);
    std::vector<double> hyp_T(head[8] ? 12 * nh : 0);
    std::vector<uint8_t> inlier(nf ? nf : 1);
    if (!get(in, slots) || !get(in, octave) || !get(in, world) || !get(in, kx) || !get(in, ky) || !get(in, sigma2) || !get(in, sets))
      return 3;
    vsg_mlpnp_result res;
    int n = 0;
    const int32_t ok = mc_args_ok(head[0], slots.data(), head[2], sigma2.data(), head[3], octave.data(), fl[0], head[4], head[5],
                                  head[6], head[7], head[1], sets.data(), inlier.data(), &res, &n);
    if (fwrite(&ok, 4, 1, out) != 1) return 4;
    if (!ok) continue;
    mc_ransac(head[0], slots.data(), world.data(), kx.data(), ky.data(), octave.data(), fl + 1, sigma2.data(), fl[0], head[4], head[5],
              head[6], head[7], head[1], sets.data(), n, inlier.data(), &res, head[8] ? hyp_inliers.data() : nullptr,
              head[8] ? hyp_T.data() : nullptr);
    inlier.resize(nf);
    if (!put(out, inlier) || fwrite(&res, sizeof res, 1, out) != 1 || !put(out, hyp_inliers) || !put(out, hyp_T)) return 4;
  }
  return fclose(out) == 0 && fclose(in) == 0 ? 0 : 4;
}
