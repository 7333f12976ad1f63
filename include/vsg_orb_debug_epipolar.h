/* vsg_orb_debug_epipolar.h -- test hook of the epipolar predicate of SearchForTriangulation (csrc/vsg_epipolar.h).  Like
 * include/vsg_orb_debug.h it is NOT part of the drop-in boundary: nothing a maintainer of the reference binds.  It has a
 * header of its own because the hooks of vsg_orb_debug.h are a closed list (tests/test_abi.py names them one by one); the
 * symbol is exported by the same library so that the tests exercise the shipped code object. */
#ifndef VSG_ORB_DEBUG_EPIPOLAR_H
#define VSG_ORB_DEBUG_EPIPOLAR_H
#include "vsg_orb.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Why the device predicate of vsg_frame_search_for_triangulation_epipolar does not take a pair as a candidate */
enum {
  VSG_EPIPOLAR_PASS = 0,         /* it does */
  VSG_EPIPOLAR_NOT_STEREO = 1,   /* bOnlyStereo and a mono keypoint on either side (ORBmatcher.cc:976-980, :1004-1008) */
  VSG_EPIPOLAR_EPIPOLE_GATE = 2, /* both mono and closer to the epipole than 100 * mvScaleFactors2[octave2] (:1023-1031) */
  VSG_EPIPOLAR_DEN_ZERO = 3,     /* a * a + b * b == 0 (Pinhole.cpp:135-136) */
  VSG_EPIPOLAR_CHI_SQUARE = 4    /* !(dsqr < 3.84 * unc), a NaN included (Pinhole.cpp:140) */
};

/* Test hook: runs the device predicate on the n listed pairs (i1[p] = feature of kf1, i2[p] = feature of kf2; the map-point
 * flags play no part) and returns the reason code of each.  Arguments and checks as
 * vsg_frame_search_for_triangulation_epipolar; an index outside its frame is VSG_ERR_INVALID before anything is enqueued. */
int vsg_debug_epipolar_pairs(vsg_frame *kf1, vsg_frame *kf2, int n, const int32_t *i1, const int32_t *i2,
                             const float F12[9], const float ep[2], const float *scale_factors2,
                             const float *level_sigma2_2, int nlevels, int only_stereo, int coarse, uint8_t *reason);

#ifdef __cplusplus
}
#endif
#endif
