// Stand-alone driver of the host core (triangulatecore.cpp: the argument check and vsg::new_points_loop) for
// tests/test_sanitizers_triangulation.py, built with AddressSanitizer + UndefinedBehaviorSanitizer linked in.
//   triangulate_sanitized IN OUT
// IN holds records until its end:
//   int32 n1, n2, nlevels, capacity (0: geometry only), n_free | vsg_triangulation_params |
//   frame 1: x y uright (n1 floats each), stereo 4 n1 floats, octave n1 (i32), desc 32 n1 bytes, scale_factors nlevels,
//   level_sigma2 nlevels | frame 2 the same with n2 | matches12 n1 (i32) | free_slots n_free (i32) |
//   with a store: pos 3 cap, normal 3 cap, min_dist cap, max_dist cap floats, desc 32 cap, observed cap bytes
// OUT gets per record: int32 ok (the argument check), and when ok: int32 n_created, reason n1, source n1, x3d 3 n1, new_slot n1
// and the store's six arrays after the loop.  Every array is a heap block of exactly its size, so a step past an end is
// reported; a record the check refuses never reaches the loop.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/vsg_orb.h"

extern "C" {
int tc_args_ok(int n1, int n2, const int32_t *matches12, const int32_t *octave1, const int32_t *octave2, int nlevels, int capacity,
               const int32_t *free_slots, int n_free);
int tc_loop(const vsg_triangulation_params *P, int n1, const float *const *f1, const int32_t *octave1, const uint8_t *desc1, int n2,
            const float *const *f2, const int32_t *octave2, const uint8_t *desc2, const int32_t *matches12, int nlevels,
            float *const *store_f, uint8_t *const *store_b, const int32_t *free_slots, int n_free, uint8_t *reason, uint8_t *source,
            float *x3d, int32_t *new_slot);
}

template <class T>
static bool get(FILE *f, std::vector<T> &a) {
  return a.empty() || fread(a.data(), sizeof(T), a.size(), f) == a.size();
}
template <class T>
static bool put(FILE *f, const std::vector<T> &a) {
  return a.empty() || fwrite(a.data(), sizeof(T), a.size(), f) == a.size();
}

struct Frame {
  std::vector<float> x, y, ur, stereo, sf, sigma2;
  std::vector<int32_t> octave;
  std::vector<uint8_t> desc;
  Frame(size_t n, size_t nl) : x(n), y(n), ur(n), stereo(4 * n), sf(nl), sigma2(nl), octave(n), desc(32 * n) {}
  bool read(FILE *f) { return get(f, x) && get(f, y) && get(f, ur) && get(f, stereo) && get(f, octave) && get(f, desc) && get(f, sf) && get(f, sigma2); }
};

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int32_t head[5];
  while (fread(head, sizeof(head), 1, in) == 1) {
    if (head[0] < 0 || head[1] < 0 || head[2] < 1 || head[2] > 16 || head[3] < 0 || head[4] < 0) return 3;
    const size_t n1 = (size_t)head[0], n2 = (size_t)head[1], nl = (size_t)head[2], cap = (size_t)head[3], nf = (size_t)head[4];
    vsg_triangulation_params P;
    if (fread(&P, sizeof P, 1, in) != 1) return 3;
    Frame A(n1, nl), B(n2, nl);
    std::vector<int32_t> matches(n1), free_slots(nf), new_slot(n1);
    if (!A.read(in) || !B.read(in) || !get(in, matches) || !get(in, free_slots)) return 3;
    std::vector<float> pos(3 * cap), normal(3 * cap), mn(cap), mx(cap), x3d(3 * n1);
    std::vector<uint8_t> desc(32 * cap), observed(cap), reason(n1), source(n1);
    if (!get(in, pos) || !get(in, normal) || !get(in, mn) || !get(in, mx) || !get(in, desc) || !get(in, observed)) return 3;
    const int32_t ok = tc_args_ok(head[0], head[1], matches.data(), A.octave.data(), B.octave.data(), head[2], head[3],
                                  free_slots.data(), head[4]);
    if (fwrite(&ok, 4, 1, out) != 1) return 4;
    if (!ok) continue;
    const float *f1[6] = {A.x.data(), A.y.data(), A.ur.data(), A.stereo.data(), A.sf.data(), A.sigma2.data()};
    const float *f2[6] = {B.x.data(), B.y.data(), B.ur.data(), B.stereo.data(), B.sf.data(), B.sigma2.data()};
    float *sf[4] = {cap ? pos.data() : nullptr, normal.data(), mn.data(), mx.data()};
    uint8_t *sb[2] = {desc.data(), observed.data()};
    const int32_t created = tc_loop(&P, head[0], f1, A.octave.data(), A.desc.data(), head[1], f2, B.octave.data(), B.desc.data(),
                                    matches.data(), head[2], sf, sb, free_slots.data(), head[4], reason.data(), source.data(),
                                    x3d.data(), new_slot.data());
    if (fwrite(&created, 4, 1, out) != 1 || !put(out, reason) || !put(out, source) || !put(out, x3d) || !put(out, new_slot) ||
        !put(out, pos) || !put(out, normal) || !put(out, mn) || !put(out, mx) || !put(out, desc) || !put(out, observed))
      return 4;
  }
  return fclose(out) == 0 && fclose(in) == 0 ? 0 : 4;
}
