// vsg_project.h -- the geometry of the two ORBmatcher searches of Tracking that project map points through the current
// pose of a Frame, for ONE map point, host and device from one source:
//   SearchByProjection(CurrentFrame, LastFrame, th, bMono)                   ORBmatcher.cc:1667-1748
//   SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist)        ORBmatcher.cc:1880-1930
// k_project_points (vsg_mappoints.hip) runs them one lane per query; tests/_projectcore and the latency probe's
// caller-side loop compile them for the host.  As in vsg_frustum.h the order is fixed and nothing contracts: every
// operation is one vsg::f* call = one rounding.
#pragma once
#include "vsg_frustum.h"

namespace vsg {

struct ImageBounds {
  float minX, maxX, minY, maxY;  // mnMinX, mnMaxX, mnMinY, mnMaxY
};

struct ProjectOut {
  int valid;       // the point reaches GetFeaturesInArea
  float u, v;      // uv                          (meaningful only when valid)
  float ur;        // uv(0) - mbf * invzc         (last-frame form)
  int level;       // nPredictedLevel             (KeyFrame form)
};

// x3Dc = Tcw * x3Dw (:1695, :1905), the rows in the order of frustum_point
VSG_HD void camera_point(const vsg_frame_pose &cam, const float *P, float *X, float *Y, float *Z) {
  *X = fadd(dot3(cam.Rcw[0], cam.Rcw[1], cam.Rcw[2], P[0], P[1], P[2]), cam.tcw[0]);
  *Y = fadd(dot3(cam.Rcw[3], cam.Rcw[4], cam.Rcw[5], P[0], P[1], P[2]), cam.tcw[1]);
  *Z = fadd(dot3(cam.Rcw[6], cam.Rcw[7], cam.Rcw[8], P[0], P[1], P[2]), cam.tcw[2]);
}

// The last-frame search's projection of pMP->GetWorldPos() (:1694-1709) and the ur of its stereo gate (:1744).
VSG_HD ProjectOut project_last_point(const vsg_frame_pose &cam, const ImageBounds &b, const float *P) {
  ProjectOut o = {0, 0.0f, 0.0f, 0.0f, 0};
  float X, Y, Z;
  camera_point(cam, P, &X, &Y, &Z);
  // :1699 `const float invzc = 1.0 / x3Dc(2)` divides in double and rounds to float.  For ONE division of floats the
  // double quotient carries 53 >= 2 * 24 + 2 bits, so rounding it again gives the correctly rounded float quotient.
  const float invzc = fdiv(1.0f, Z);
  if (invzc < 0.0f) return o;  // :1701-1702 (Z == +0 and NaN go on)
  // Pinhole::project (Pinhole.cpp:46-53): fx * X / Z + cx
  const float u = fadd(fdiv(fmul(cam.fx, X), Z), cam.cx);
  const float v = fadd(fdiv(fmul(cam.fy, Y), Z), cam.cy);
  if (u < b.minX || u > b.maxX) return o;  // :1706-1709 (a NaN passes, as in the reference)
  if (v < b.minY || v > b.maxY) return o;
  o.valid = 1, o.u = u, o.v = v;
  o.ur = fsub(u, fmul(cam.mbf, invzc));  // :1744
  return o;
}

// The relocalisation search's projection (:1904-1925): NO sign test on the depth (the reference has none here), the
// distance band of the getters and MapPoint::PredictScale on the member mfMaxDistance.
VSG_HD ProjectOut project_kf_point(const vsg_frame_pose &cam, const ImageBounds &b, const float *P, float mfMinDistance,
                                   float mfMaxDistance) {
  ProjectOut o = {0, 0.0f, 0.0f, 0.0f, 0};
  float X, Y, Z;
  camera_point(cam, P, &X, &Y, &Z);
  const float u = fadd(fdiv(fmul(cam.fx, X), Z), cam.cx);  // :1907
  const float v = fadd(fdiv(fmul(cam.fy, Y), Z), cam.cy);
  if (u < b.minX || u > b.maxX) return o;  // :1909-1912
  if (v < b.minY || v > b.maxY) return o;
  const float PO0 = fsub(P[0], cam.Ow[0]), PO1 = fsub(P[1], cam.Ow[1]), PO2 = fsub(P[2], cam.Ow[2]);  // :1915
  const float dist3D = fsqrt(dot3(PO0, PO1, PO2, PO0, PO1, PO2));                                       // :1916
  // GetMaxDistanceInvariance() = 1.2f * mfMaxDistance, GetMinDistanceInvariance() = 0.8f * mfMinDistance (MapPoint.cc:521-531)
  const float maxDistance = fmul(1.2f, mfMaxDistance), minDistance = fmul(0.8f, mfMinDistance);  // :1918-1919
  if (dist3D < minDistance || dist3D > maxDistance) return o;                                    // :1922-1923
  o.valid = 1, o.u = u, o.v = v;
  o.level = predict_scale(mfMaxDistance, dist3D, cam.log_scale_factor, cam.n_levels);  // :1925
  return o;
}

// bForward / bBackward (:1677-1684): tlc = Tlw * twc with twc = the current pose's Ow (mOw = Twc.translation()); only its z
// is used.  1 = forward, 2 = backward, 0 = neither.
VSG_HD int motion_direction(const vsg_frame_pose &cur, const vsg_frame_pose &last, float mb, int mono) {
  const float tlc_z = fadd(dot3(last.Rcw[6], last.Rcw[7], last.Rcw[8], cur.Ow[0], cur.Ow[1], cur.Ow[2]), last.tcw[2]);
  if (tlc_z > mb && !mono) return 1;
  if (-tlc_z > mb && !mono) return 2;
  return 0;
}

}  // namespace vsg
