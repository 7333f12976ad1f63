// vsg_frustum.h -- Frame::isInFrustum (Frame.cc:656-719, the Nleft == -1 branch) for ONE map point, host and device
// from one source: k_frustum (vsg_mappoints.hip) runs it one lane per point, tests/_frustumcore and the latency probe's
// caller-side loop (tools/resident_points_cpu.cpp) compile it for the host.
//
// The reference evaluates this in Eigen float under -O3 -march=native, so its bits follow the compiler's contraction;
// here the order is fixed and nothing contracts: every operation is one vsg::f* call = one rounding.
#pragma once
#include "../../include/vsg_orb.h"
#include "vsg_math.h"

namespace vsg {

struct FrustumOut {
  int in_view;              // mbTrackInView
  float proj_x, proj_y;     // mTrackProjX / Y: -1 until :684, u / v from there on
  float proj_xr, depth;     // mTrackProjXR, mTrackDepth     (the rest: meaningful only when in_view)
  int scale_level;          // mnTrackScaleLevel
  float view_cos;           // mTrackViewCos
};

// MapPoint::PredictScale (MapPoint.cc:550-565): ceil(log(mfMaxDistance / currentDist) / mfLogScaleFactor), clamped.
// mfMaxDistance is the member, NOT the 1.2f * mfMaxDistance that GetMaxDistanceInvariance() returns.
VSG_HD int predict_scale(float mfMaxDistance, float dist, float log_scale_factor, int n_levels) {
  const float ratio = fdiv(mfMaxDistance, dist);
  int nScale = cvt_int_x86(__builtin_ceilf(fdiv(log_f32(ratio), log_scale_factor)));
  if (nScale < 0)
    nScale = 0;
  else if (nScale >= n_levels)
    nScale = n_levels - 1;
  return nScale;
}

VSG_HD float dot3(float a0, float a1, float a2, float b0, float b1, float b2) {
  return fadd(fadd(fmul(a0, b0), fmul(a1, b1)), fmul(a2, b2));
}

// P = GetWorldPos(), Pn = GetNormal(), mfMinDistance / mfMaxDistance = the MapPoint's members; bounds = mnMinX..mnMaxY
VSG_HD FrustumOut frustum_point(const vsg_frame_pose &cam, float minX, float maxX, float minY, float maxY,
                                float viewing_cos_limit, float P0, float P1, float P2, float n0, float n1, float n2,
                                float mfMinDistance, float mfMaxDistance) {
  FrustumOut o = {0, -1.0f, -1.0f, 0.0f, 0.0f, 0, 0.0f};  // :660-662
  // Pc = mRcw * P + mtcw (:668), Pc.norm() (:669)
  const float PcX = fadd(dot3(cam.Rcw[0], cam.Rcw[1], cam.Rcw[2], P0, P1, P2), cam.tcw[0]);
  const float PcY = fadd(dot3(cam.Rcw[3], cam.Rcw[4], cam.Rcw[5], P0, P1, P2), cam.tcw[1]);
  const float PcZ = fadd(dot3(cam.Rcw[6], cam.Rcw[7], cam.Rcw[8], P0, P1, P2), cam.tcw[2]);
  const float Pc_dist = fsqrt(dot3(PcX, PcY, PcZ, PcX, PcY, PcZ));
  const float invz = fdiv(1.0f, PcZ);  // :673
  if (PcZ < 0.0f) return o;            // :674-675 (0 and NaN go on)
  // Pinhole::project (Pinhole.cpp:46-53): fx * X / Z + cx
  const float u = fadd(fdiv(fmul(cam.fx, PcX), PcZ), cam.cx);
  const float v = fadd(fdiv(fmul(cam.fy, PcY), PcZ), cam.cy);
  if (u < minX || u > maxX) return o;  // :679-682 (a NaN passes, as in the reference)
  if (v < minY || v > maxY) return o;
  o.proj_x = u, o.proj_y = v;  // :684-685
  const float PO0 = fsub(P0, cam.Ow[0]), PO1 = fsub(P1, cam.Ow[1]), PO2 = fsub(P2, cam.Ow[2]);  // :690
  const float dist = fsqrt(dot3(PO0, PO1, PO2, PO0, PO1, PO2));
  // GetMaxDistanceInvariance() = 1.2f * mfMaxDistance, GetMinDistanceInvariance() = 0.8f * mfMinDistance (MapPoint.cc:521-531)
  const float maxDistance = fmul(1.2f, mfMaxDistance), minDistance = fmul(0.8f, mfMinDistance);  // :688-689
  if (dist < minDistance || dist > maxDistance) return o;  // :693-694
  const float viewCos = fdiv(dot3(PO0, PO1, PO2, n0, n1, n2), dist);  // :699
  if (viewCos < viewing_cos_limit) return o;                          // :701-702
  o.scale_level = predict_scale(mfMaxDistance, dist, cam.log_scale_factor, cam.n_levels);  // :705
  o.in_view = 1;
  o.proj_xr = fsub(u, fmul(cam.mbf, invz));  // :710
  o.depth = Pc_dist;
  o.view_cos = viewCos;
  return o;
}

}  // namespace vsg
