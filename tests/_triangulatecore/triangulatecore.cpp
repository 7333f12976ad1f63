// Host build of the loop body of LocalMapping::CreateNewMapPoints (vsg_triangulate.h), for tests/triangulation_hostcore.py:
// the same source k_new_points compiles, against the NumPy restatement and against the device.
#include "vsg_triangulate.h"

#include <vector>

extern "C" {

int tc_params_size() { return (int)sizeof(vsg_triangulation_params); }

// the right singular vector of the least singular value of n 4 x 4 float matrices (double, before the rounding to float)
void tc_null_vectors(int n, const float *A, double *v) {
  for (int i = 0; i < n; i++) vsg::tri_null_vector(A + 16 * (size_t)i, v + 4 * (size_t)i);
}

// vsg::triangulate_pair for n pairs; f1 / f2 = n x vsg::TriFeature (9 floats each)
void tc_pairs(int n, const vsg_triangulation_params *P, const float *f1, const float *f2, uint8_t *reason, uint8_t *source,
              float *x3d) {
  static_assert(sizeof(vsg::TriFeature) == 36, "TriFeature is 9 floats");
  for (int i = 0; i < n; i++) {
    const vsg::TriOut o = vsg::triangulate_pair(*P, ((const vsg::TriFeature *)f1)[i], ((const vsg::TriFeature *)f2)[i]);
    reason[i] = (uint8_t)o.reason, source[i] = (uint8_t)o.source;
    for (int k = 0; k < 3; k++) x3d[3 * (size_t)i + k] = o.x3D[k];
  }
}

// rays and parallax of n pairs: out = n x {ray1[3], ray2[3], cosParallaxRays}
void tc_parallax(int n, const vsg_triangulation_params *P, const float *f1, const float *f2, float *out) {
  for (int i = 0; i < n; i++) {
    float xn1[3], xn2[3];
    float *o = out + 7 * (size_t)i;
    o[6] = vsg::tri_cos_parallax_rays(P->kf1, P->kf2, ((const vsg::TriFeature *)f1)[i], ((const vsg::TriFeature *)f2)[i], xn1, xn2, o,
                                      o + 3);
  }
}

void tc_normal_and_depth(const vsg_triangulation_params *P, const float *x3D, int octave1, const float *scale_factors1, int nlevels,
                         float *normal, float *min_dist, float *max_dist) {
  vsg::new_point_normal_and_depth(*P, x3D, octave1, scale_factors1, nlevels, normal, min_dist, max_dist);
}

// what the entry points refuse before they enqueue, as far as it needs no device: 1 = the arguments pass
int tc_args_ok(int n1, int n2, const int32_t *matches12, const int32_t *octave1, const int32_t *octave2, int nlevels,
               int capacity, const int32_t *free_slots, int n_free) {
  if (nlevels < 1 || nlevels > 16 || n1 < 0 || n2 < 0 || (n1 > 0 && !matches12)) return 0;
  if (!vsg::tri_octaves_ok(n1, [&](int i) { return octave1[i]; }, nlevels)) return 0;
  if (!vsg::tri_octaves_ok(n2, [&](int i) { return octave2[i]; }, nlevels)) return 0;
  if (!vsg::tri_matches_ok(n1, n2, matches12)) return 0;
  if (capacity > 0) {
    std::vector<uint8_t> seen((size_t)capacity, 0);
    if (!vsg::tri_free_slots_ok(capacity, free_slots, n_free, seen.data())) return 0;
  }
  return 1;
}

// vsg::new_points_loop.  frame k = {x, y, uright (may be NULL), stereo (may be NULL), scale_factors, level_sigma2} as floats,
// octave, desc; store = {pos, normal, min_dist, max_dist} and {desc, observed}, all NULL for geometry only.
int tc_loop(const vsg_triangulation_params *P, int n1, const float *const *f1, const int32_t *octave1, const uint8_t *desc1,
            int n2, const float *const *f2, const int32_t *octave2, const uint8_t *desc2, const int32_t *matches12, int nlevels,
            float *const *store_f, uint8_t *const *store_b, const int32_t *free_slots, int n_free, uint8_t *reason,
            uint8_t *source, float *x3d, int32_t *new_slot) {
  const vsg::TriFrameHost A{n1, f1[0], f1[1], octave1, f1[2], f1[3], desc1, f1[4], f1[5]};
  const vsg::TriFrameHost B{n2, f2[0], f2[1], octave2, f2[2], f2[3], desc2, f2[4], f2[5]};
  vsg::TriStoreHost S{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  if (store_f && store_f[0]) S = {store_f[0], store_f[1], store_f[2], store_f[3], store_b[0], store_b[1]};
  return vsg::new_points_loop(*P, A, B, matches12, nlevels, S, free_slots, n_free, reason, source, x3d, new_slot);
}
}
