// Host build of the epipolar predicate of SearchForTriangulation (vsg_epipolar.h), for tests/test_epipolar_reference.py:
// the same source k_triangulation_walk<EpipolarPred> compiles, against the NumPy restatement.
#include "vsg_epipolar.h"

extern "C" {

// vsg::epipolar_reason_pair for n pairs; scale_factors2 / level_sigma2_2 are indexed by octave2 (the caller checked it)
void ec_pair_reasons(int n, const float *x1, const float *y1, const float *ur1, const float *x2, const float *y2,
                     const float *ur2, const int32_t *octave2, const float *F12, const float *ep,
                     const float *scale_factors2, const float *level_sigma2_2, int only_stereo, int coarse,
                     uint8_t *reason) {
  for (int i = 0; i < n; i++)
    reason[i] = (uint8_t)vsg::epipolar_reason_pair(F12, ep, x1[i], y1[i], ur1[i], x2[i], y2[i], ur2[i],
                                                   scale_factors2[octave2[i]], level_sigma2_2[octave2[i]], only_stereo, coarse);
}

// the two per-level values the kernel keeps in tables
float ec_gate_radius(float scale_factor) { return vsg::epipole_gate_radius(scale_factor); }
double ec_chi_square_bound(float level_sigma2) { return vsg::chi_square_bound(level_sigma2); }
}
