// vsg_windows.h -- the GetFeaturesInArea window of every ORBmatcher search routine as ONE WinQuery builder, host and
// device from one source: the host-array entry points (vsg_window.hip) fill their queries with these, k_frustum and
// k_project_points (vsg_mappoints.hip) call the same ones one lane per map point.  Line numbers are ORBmatcher.cc's.
// As in vsg_frustum.h every operation is one vsg::f* call = one rounding.  Builders do not validate: a level or an
// octave indexes scale_factors as it is, the callers refuse what lies outside the pyramid.
#pragma once
#include <stdint.h>

#include "vsg_math.h"

namespace vsg {

// One GetFeaturesInArea window + the static candidate filters of a search routine.
struct WinQuery {
  float x, y, r;    // Frame::GetFeaturesInArea(x, y, r, minLevel, maxLevel, bRight)   (Frame.cc:802-868)
  int minL, maxL;   //   (-1, -1 = KeyFrame::GetFeaturesInArea, KeyFrame.cc:834-874)
  int lo, hi;       // kpLevel < lo || kpLevel > hi -> skip (hi < 0: no such filter)       e.g. :506-509
  float ur, gate;   // projected right coordinate + threshold of the stereo gates           e.g. :97-102
  int flags;        // kWinRight | kWinInactive
  int pad0, pad1;
};
static_assert(sizeof(WinQuery) == 48, "WinQuery layout");
enum { kWinRight = 1,       // bRight: mGridRight, indices + Nleft
       kWinInactive = 2 };  // the routine `continue`s before GetFeaturesInArea: empty list

// Frame::GetFeaturesInArea(x, y, r, minL, maxL, bRight) and nothing else: no level filter, no stereo gate
// (the one place that spells a WinQuery out field by field: everything else starts from this and names what it sets)
VSG_HD WinQuery win_area(float x, float y, float r, int minL, int maxL, bool right, bool inactive = false) {
  const int flags = (right ? kWinRight : 0) | (inactive ? kWinInactive : 0);
  return {x, y, r, minL, maxL, /*lo, hi*/ 0, -1, /*ur, gate*/ 0.f, 0.f, flags, 0, 0};
}
VSG_HD WinQuery win_inactive(bool right) { return win_area(0.f, 0.f, 0.f, -1, -1, right, true); }

// ORBmatcher::RadiusByViewingCos (:218-224); the comparison is with the double 0.998
VSG_HD float radius_by_viewing_cos(float viewCos) { return (double)viewCos > 0.998 ? 2.5f : 4.0f; }

// SearchByProjection(F, vpMapPoints, th, bFarPoints, thFarPoints), left block:
// GetFeaturesInArea(mTrackProjX, mTrackProjY, r * mvScaleFactors[level], level - 1, level) (:69-70) with
// r = RadiusByViewingCos(mTrackViewCos) (:64), r *= th when bFactor (:66-67); xr and the window as the gate of :97-102
VSG_HD WinQuery win_local(float x, float y, float xr, int level, float view_cos, float th, bool b_factor,
                          const float *scale_factors) {
  float r = radius_by_viewing_cos(view_cos);
  if (b_factor) r = fmul(r, th);
  const float win = fmul(r, scale_factors[level]);
  WinQuery w = win_area(x, y, win, level - 1, level, false);
  w.ur = xr, w.gate = win;
  return w;
}

// ... right block (:151-157): no th factor, no ur, no gate
VSG_HD WinQuery win_local_right(float x, float y, int level, float view_cos, const float *scale_factors) {
  return win_area(x, y, fmul(radius_by_viewing_cos(view_cos), scale_factors[level]), level - 1, level, true);
}

// SearchByProjection(CurrentFrame, LastFrame, th, bMono): radius = th * mvScaleFactors[nLastOctave] (:1714-1715);
// level window (:1718-1724): forward -> (nLastOctave, -1), backward -> (0, nLastOctave), else +-1.
// direction: 0 neither, 1 bForward, 2 bBackward.  This alone is the right block's query (:1797-1803): no stereo gate
VSG_HD WinQuery win_last_area(float u, float v, int octave, float th, int direction, const float *scale_factors,
                              bool right) {
  const int minL = direction == 1 ? octave : direction == 2 ? 0 : octave - 1;
  const int maxL = direction == 1 ? -1 : direction == 2 ? octave : octave + 1;
  return win_area(u, v, fmul(th, scale_factors[octave]), minL, maxL, right);
}
// left block: ur and the radius as the gate of :1741-1747 (the gate is carried whether or not the call has a ur)
VSG_HD WinQuery win_last(float u, float v, float ur, int octave, float th, int direction, const float *scale_factors) {
  WinQuery w = win_last_area(u, v, octave, th, direction, scale_factors, false);
  w.ur = ur, w.gate = w.r;
  return w;
}

// SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist): GetFeaturesInArea(u, v, radius, l - 1, l + 1) (:1930-1934)
VSG_HD WinQuery win_kf(float u, float v, float radius, int l) { return win_area(u, v, radius, l - 1, l + 1, false); }

// pKF->GetFeaturesInArea(u, v, radius, bRight) followed by kpLevel in [level - 1, level]: the Sim3 SearchByProjection
// (:485, :506-509), SearchBySim3 (:1531 / :1609, :1547-1548 / :1625-1626) and Fuse (:1240 / :1394, :1262-1265 /
// :1411-1414; ur for its chi-square gate).  Inactive when level < 0.
VSG_HD WinQuery win_keyframe_area(float u, float v, float radius, int level, float ur, bool right) {
  WinQuery w = win_area(u, v, radius, -1, -1, right, level < 0);
  w.lo = level - 1, w.hi = level, w.ur = ur;
  return w;
}

}  // namespace vsg
