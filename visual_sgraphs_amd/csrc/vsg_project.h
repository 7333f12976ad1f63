// vsg_project.h -- the geometry of the ORBmatcher routines that project map points through a pose, for ONE map point,
// host and device from one source.  Tracking's two searches through the current pose of a Frame:
//   SearchByProjection(CurrentFrame, LastFrame, th, bMono)                   ORBmatcher.cc:1667-1748
//   SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist)        ORBmatcher.cc:1880-1930
// and the back end's four routines that project into a KeyFrame (project_keyframe_point: one loop, written four times):
//   SearchByProjection(pKF, Scw, vpPoints, vpMatched, th, ratioHamming) x2   ORBmatcher.cc:452-486, :559-595
//   Fuse(pKF, vpMapPoints, th, bRight)                                       ORBmatcher.cc:1194-1241
//   Fuse(pKF, Scw, vpPoints, th, vpReplacePoint)                             ORBmatcher.cc:1360-1395
// k_project_points (vsg_mappoints.hip) runs them one lane per query; tests/_projectcore, tests/_keyframecore and the
// latency probe's caller-side loops (tools/resident_points_cpu.cpp) compile them for the host.  As in vsg_frustum.h the order is fixed and nothing contracts: every
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
  float ur;        // uv(0) - mbf * invzc         (last-frame form, project_keyframe_point)
  int level;       // nPredictedLevel             (the two KeyFrame forms)
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

// KeyFrame::mnMinX .. mnMaxY are `const int` (KeyFrame.h:419-422) initialised from the Frame's floats (KeyFrame.cc:52):
// truncation toward zero.  IsInImage compares a float with them, i.e. with the int converted back to float.
VSG_HD ImageBounds keyframe_bounds(const ImageBounds &frame) {
  return {(float)cvt_int_x86(frame.minX), (float)cvt_int_x86(frame.maxX), (float)cvt_int_x86(frame.minY),
          (float)cvt_int_x86(frame.maxY)};
}

// The per-point loop of Fuse(pKF, vpMapPoints, th) (:1194-1238), which is also that of Fuse(pKF, Scw, ...) (:1360-1392)
// and of the two SearchByProjection(pKF, Scw, ...) (:452-483, :559-592) once those have decomposed Scw into Tcw / Ow
// (:433-434, :1340-1341); only Fuse's pose form reads ur.  kf = keyframe_bounds() of the resident frame's bounds.
VSG_HD ProjectOut project_keyframe_point(const vsg_frame_pose &cam, const ImageBounds &kf, const float *P, const float *Pn,
                                         float mfMinDistance, float mfMaxDistance) {
  ProjectOut o = {0, 0.0f, 0.0f, 0.0f, 0};
  float X, Y, Z;
  camera_point(cam, P, &X, &Y, &Z);  // :1195
  if (Z < 0.0f) return o;            // :1198 (0 and NaN go on)
  const float invz = fdiv(1.0f, Z);  // :1204
  // Pinhole::project (Pinhole.cpp:46-53): fx * X / Z + cx
  const float u = fadd(fdiv(fmul(cam.fx, X), Z), cam.cx);  // :1206
  const float v = fadd(fdiv(fmul(cam.fy, Y), Z), cam.cy);
  // KeyFrame::IsInImage (KeyFrame.cc:880-883): the maximum is exclusive and a NaN is rejected
  if (!(u >= kf.minX && u < kf.maxX && v >= kf.minY && v < kf.maxY)) return o;  // :1209
  const float ur = fsub(u, fmul(cam.mbf, invz));                                 // :1215
  const float PO0 = fsub(P[0], cam.Ow[0]), PO1 = fsub(P[1], cam.Ow[1]), PO2 = fsub(P[2], cam.Ow[2]);  // :1219
  const float dist3D = fsqrt(dot3(PO0, PO1, PO2, PO0, PO1, PO2));                                       // :1220
  // GetMaxDistanceInvariance() = 1.2f * mfMaxDistance, GetMinDistanceInvariance() = 0.8f * mfMinDistance (MapPoint.cc:521-531)
  const float maxDistance = fmul(1.2f, mfMaxDistance), minDistance = fmul(0.8f, mfMinDistance);  // :1217-1218
  if (dist3D < minDistance || dist3D > maxDistance) return o;                                    // :1223
  // :1232 `PO.dot(Pn) < 0.5 * dist3D`: the float dot product against a double product (exact: a halving)
  if ((double)dot3(PO0, PO1, PO2, Pn[0], Pn[1], Pn[2]) < dmul(0.5, (double)dist3D)) return o;
  o.valid = 1, o.u = u, o.v = v, o.ur = ur;
  o.level = predict_scale(mfMaxDistance, dist3D, cam.log_scale_factor, cam.n_levels);  // :1238
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
