// vsg_epipolar.h -- the geometric predicate of ORBmatcher::SearchForTriangulation (ORBmatcher.cc:976-1073) for ONE pair of
// keypoints (kp1 of pKF1, kp2 of pKF2), host and device from one source: the stereo test of `bOnlyStereo` (:976-980,
// :1004-1008), the epipole distance gate (:1023-1031) and `bCoarse || Pinhole::epipolarConstrain` (:1073,
// Pinhole.cpp:118-141).  k_triangulation_walk<EpipolarPred> and k_epipolar_pairs (vsg_match.hip) run it on the device;
// tests/_epipolarcore, tests/_adaptor_triangulation and the latency probe's caller-side loop (tools/abi_latency.cpp)
// compile it for the host.  As in vsg_frustum.h / vsg_project.h the order is fixed and nothing contracts: every operation
// is one vsg::f* / vsg::d* call = one rounding.
//
// F12 (row-major: F12(r, c) = F12[3 * r + c]) and the epipole ep are INPUTS.  The reference builds F12 with Eigen inside
// epipolarConstrain (Pinhole.cpp:121-124: K1.transpose().inverse() * hat(t12) * R12 * K2.inverse()) and ep at
// ORBmatcher.cc:913-915 (pKF2->mpCamera->project(T2w * Cw)); both depend on the pair of KEYFRAMES only, so the caller computes
// them once per call with the reference's own expressions: nothing here restates an Eigen inverse.  epipolarConstrain's
// `sigmaLevel` argument is not used by Pinhole and is not taken.
#pragma once
#include "vsg_math.h"

namespace vsg {

// why a pair is not a candidate (0: it is one); the tests compare these
enum { kEpiPass = 0, kEpiNotStereo = 1, kEpiEpipoleGate = 2, kEpiDenZero = 3, kEpiChiSquare = 4 };

// what the predicate reads of one pyramid level of pKF2: `100 * pKF2->mvScaleFactors[kp2.octave]` in float (:1027: the int
// 100 converts to float) and `3.84 * unc` in DOUBLE (Pinhole.cpp:140: unc = pKF2->mvLevelSigma2[kp2.octave] promotes)
VSG_HD float epipole_gate_radius(float scale_factor) { return fmul(100.0f, scale_factor); }
VSG_HD double chi_square_bound(float level_sigma2) { return dmul(3.84, (double)level_sigma2); }

// Epipolar line in the second image l = x1' F12 = [a b c] (Pinhole.cpp:127-129) and den = a * a + b * b (:133): they depend
// on kp1 alone, so a kernel keeps them per KF1 feature
struct EpipolarLine {
  float a, b, c, den;
};
VSG_HD EpipolarLine epipolar_line(const float *F12, float x1, float y1) {
  EpipolarLine l;
  l.a = fadd(fadd(fmul(x1, F12[0]), fmul(y1, F12[3])), F12[6]);
  l.b = fadd(fadd(fmul(x1, F12[1]), fmul(y1, F12[4])), F12[7]);
  l.c = fadd(fadd(fmul(x1, F12[2]), fmul(y1, F12[5])), F12[8]);
  l.den = fadd(fmul(l.a, l.a), fmul(l.b, l.b));
  return l;
}

// The pair's reason code.  stereo1 / stereo2 = mvuRight >= 0 (a frame without mvuRight counts as all -1); gate2 / bound2 =
// epipole_gate_radius / chi_square_bound of kp2's level.  `line` is not read when coarse is set.
VSG_HD int epipolar_reason(const EpipolarLine &line, bool stereo1, float x2, float y2, bool stereo2, float ep0, float ep1,
                           float gate2, double bound2, int only_stereo, int coarse) {
  if (only_stereo && (!stereo1 || !stereo2)) return kEpiNotStereo;  // :976-980, :1004-1008
  if (!stereo1 && !stereo2) {                                       // :1023 (also under bCoarse)
    const float distex = fsub(ep0, x2), distey = fsub(ep1, y2);
    if (fadd(fmul(distex, distex), fmul(distey, distey)) < gate2) return kEpiEpipoleGate;  // :1027
  }
  if (coarse) return kEpiPass;  // :1073
  const float num = fadd(fadd(fmul(line.a, x2), fmul(line.b, y2)), line.c);  // Pinhole.cpp:131
  if (line.den == 0) return kEpiDenZero;                                     // :135-136
  const float dsqr = fdiv(fmul(num, num), line.den);                         // :138
  return (double)dsqr < bound2 ? kEpiPass : kEpiChiSquare;                   // :140 (a NaN is not below anything: rejected)
}

// the same from the raw per-keypoint values
VSG_HD int epipolar_reason_pair(const float *F12, const float *ep, float x1, float y1, float uright1, float x2, float y2,
                                float uright2, float scale_factor2, float level_sigma2_2, int only_stereo, int coarse) {
  EpipolarLine line = {0.0f, 0.0f, 0.0f, 0.0f};
  if (!coarse) line = epipolar_line(F12, x1, y1);
  return epipolar_reason(line, uright1 >= 0, x2, y2, uright2 >= 0, ep[0], ep[1], epipole_gate_radius(scale_factor2),
                         chi_square_bound(level_sigma2_2), only_stereo, coarse);
}

}  // namespace vsg
