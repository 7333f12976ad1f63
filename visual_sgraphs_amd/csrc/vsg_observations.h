// vsg_observations.h -- MapPoint::UpdateNormalAndDepth (MapPoint.cc:440-513, every keyframe with NLeft == -1: one
// observation per keyframe, its leftIndex) for ONE map point, host and device from one source: k_refresh
// (vsg_mappoints.hip) runs it per point, tests/_obscore and the latency probe's caller-side loop
// (tools/resident_points_cpu.cpp) compile it for the host.
//
// The reference evaluates this in Eigen float under -O3 -march=native, so its bits follow the compiler's contraction;
// here the order is fixed and nothing contracts (the project's pin): every operation is one
// vsg::f* call = one rounding.  The mean viewing direction is a SERIAL sum in the order of the point's observations
// (the reference's std::map<KeyFrame *, ...> order, which the caller keeps): float addition does not associate.
#pragma once
#include "vsg_frustum.h"

namespace vsg {

// normali / normali.norm() (:471-472): a true division per component -- Eigen's vector / scalar is a quotient, not a
// product with the reciprocal.  P == Ow gives 0 / 0 = NaN, as in the reference.
VSG_HD void observation_unit(const float *P, const float *Ow, float *u) {
  const float d0 = fsub(P[0], Ow[0]), d1 = fsub(P[1], Ow[1]), d2 = fsub(P[2], Ow[2]);
  const float len = fsqrt(dot3(d0, d1, d2, d0, d1, d2));
  u[0] = fdiv(d0, len), u[1] = fdiv(d1, len), u[2] = fdiv(d2, len);
}

// normal = normal + normali / normali.norm() (:472), one observation
VSG_HD void observation_add(float *sum, const float *u) {
  sum[0] = fadd(sum[0], u[0]), sum[1] = fadd(sum[1], u[1]), sum[2] = fadd(sum[2], u[2]);
}

// mNormalVector = normal / n (:511), n = the number of observations
VSG_HD void observation_mean(const float *sum, int m, float *normal) {
  const float fm = (float)m;
  normal[0] = fdiv(sum[0], fm), normal[1] = fdiv(sum[1], fm), normal[2] = fdiv(sum[2], fm);
}

// :484-485, :504-510: PC = Pos - pRefKF->GetCameraCenter(), dist = PC.norm(); mfMaxDistance = dist *
// mvScaleFactors[level], mfMinDistance = mfMaxDistance / mvScaleFactors[nLevels - 1].  level = the octave of the
// reference keyframe's keypoint, in [0, nlevels).
VSG_HD void observation_depth(const float *P, const float *Ow_ref, const float *scale_factors, int level, int nlevels,
                              float *min_dist, float *max_dist) {
  const float c0 = fsub(P[0], Ow_ref[0]), c1 = fsub(P[1], Ow_ref[1]), c2 = fsub(P[2], Ow_ref[2]);
  const float dist = fsqrt(dot3(c0, c1, c2, c0, c1, c2));
  const float mx = fmul(dist, scale_factors[level]);
  *max_dist = mx;
  *min_dist = fdiv(mx, scale_factors[nlevels - 1]);
}

// The whole routine for a point at P with m >= 1 observations: kf[j] = the keyframe of observation j, Ow = the camera
// centres [3 per keyframe], ref = the position of mpRefKF's observation in the list, ref_level = its keypoint's octave.
VSG_HD void update_normal_and_depth(const float *P, int m, const int32_t *kf, const float *Ow, int ref, int ref_level,
                                    const float *scale_factors, int nlevels, float *normal, float *min_dist,
                                    float *max_dist) {
  float sum[3] = {0.0f, 0.0f, 0.0f};  // normal.setZero() (:459)
  for (int j = 0; j < m; j++) {
    float u[3];
    observation_unit(P, Ow + 3 * (size_t)kf[j], u);
    observation_add(sum, u);
  }
  observation_depth(P, Ow + 3 * (size_t)kf[ref], scale_factors, ref_level, nlevels, min_dist, max_dist);
  observation_mean(sum, m, normal);
}

}  // namespace vsg
