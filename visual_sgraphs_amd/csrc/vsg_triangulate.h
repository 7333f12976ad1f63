// vsg_triangulate.h -- the body of LocalMapping::CreateNewMapPoints' loop over the matches of one neighbour
// (LocalMapping.cc:475-708, both keyframes with NLeft == -1 and the Pinhole camera) for ONE matched pair (idx1 of the
// current keyframe, idx2 of pKF2), host and device from one source: k_triangulate (vsg_triangulate.hip) runs it one lane
// per feature of the current keyframe, tests/_triangulatecore and the latency probe's caller-side loop
// (tools/resident_points_cpu.cpp) compile it for the host.  As in vsg_epipolar.h / vsg_frustum.h /
// vsg_observations.h the order is fixed and nothing contracts: every operation is one vsg::f* / vsg::d* call = one
// rounding, and every comparison is written as the reference writes it, so that a NaN takes the reference's branch.
//
// INPUTS the header does not restate: cos(2 * atan2(mb / 2, mvDepth[i])) (:569, :571) and x3Dc of
// KeyFrame::UnprojectStereo (KeyFrame.cc:887-894: the RAW keypoint mvKeys[i], which a resident frame does not hold) are
// per-feature values of ONE keyframe; the caller computes them once per keyframe with the reference's own expressions
// (vsg_frame_set_stereo_points).  No libm is restated here.
//
// DEVIATION of arithmetic class: GeometricTools::Triangulate (GeometricTools.cc:47-66) takes the last right singular
// vector of the float 4 x 4 A from Eigen's float JacobiSVD, which cannot be restated bit for bit without Eigen.  Here A is
// built in float exactly as :50-53 and its right singular vector of the least singular value comes from a one-sided
// (Hestenes) Jacobi on the columns of A in DOUBLE with a compile-time number of sweeps; the result is rounded to float
// once.  DESIGN.md section 8 records it beside the LDL^T of the pose solve.
#pragma once
#include <stddef.h>

#include "../../include/vsg_orb.h"
#include "vsg_jacobi.h"
#include "vsg_math.h"
#include "vsg_observations.h"

#if defined(__HIPCC__)
#define VSG_TRI_UNROLL _Pragma("unroll")
#else
#define VSG_TRI_UNROLL
#endif

namespace vsg {

// why a pair makes no map point (0: it makes one), in the reference's order; the tests compare these
enum {
  kTriAccepted = 0,
  kTriLowParallax = 1,   // :600-603 "No stereo and very low parallax"
  kTriWZero = 2,         // GeometricTools.cc:59
  kTriStereoDepth = 3,   // KeyFrame.cc:888, :900
  kTriZ1 = 4,            // :613
  kTriZ2 = 5,            // :617
  kTriReproj1 = 6,       // :632 / :643
  kTriReproj2 = 7,       // :657 / :668
  kTriDistZero = 8,      // :679
  kTriFar = 9,           // :682
  kTriScaleRatio = 10,   // :688
  kTriNoFreeSlot = 11,   // added by the caller of this header: accepted, but the free-slot list is used up
  kTriNoMatch = 255      // the feature has no match
};
// where x3D came from (bPointStereo, countStereo: :591, :597, :693)
enum { kTriFromTriangulate = 0, kTriFromStereo1 = 1, kTriFromStereo2 = 2 };
enum { kTriSweeps = 6 };  // Hestenes sweeps: a NumPy trial reached its final accuracy (1.6e-11 of |x3D| from LAPACK) at 5

// what the loop reads of one keypoint: kpUn.pt, kpUn.octave's two table entries, mvuRight, and (read only where
// uright >= 0) the two attached stereo values
struct TriFeature {
  float x, y, uright;
  float scale_factor, level_sigma2;  // mvScaleFactors[octave], mvLevelSigma2[octave]
  float cos_stereo;                  // cos(2 * atan2(mb / 2, mvDepth[i]))
  float xyz_c[3];                    // x3Dc of UnprojectStereo
};

struct TriOut {
  int reason, source;
  float x3D[3];  // zeros until the reference has assigned it
};

// Pinhole::unprojectEig (Pinhole.cpp:66-70)
VSG_HD void tri_unproject(const vsg_frame_pose &c, float x, float y, float *xn) {
  xn[0] = fdiv(fsub(x, c.cx), c.fx), xn[1] = fdiv(fsub(y, c.cy), c.fy), xn[2] = 1.0f;
}
// Rwc * v with Rwc = Rcw transposed (:411, :560): component i sums k = 0, 1, 2 of Rcw(k, i) * v(k)
VSG_HD void tri_rotate_wc(const vsg_frame_pose &c, const float *v, float *out) {
  for (int i = 0; i < 3; i++) out[i] = fadd(fadd(fmul(c.Rcw[i], v[0]), fmul(c.Rcw[3 + i], v[1])), fmul(c.Rcw[6 + i], v[2]));
}
// Rcw.row(r).dot(x3D) + tcw(r) (:612, :622-623)
VSG_HD float tri_camera_coord(const vsg_frame_pose &c, int r, const float *X) {
  return fadd(dot3(c.Rcw[3 * r], c.Rcw[3 * r + 1], c.Rcw[3 * r + 2], X[0], X[1], X[2]), c.tcw[r]);
}
VSG_HD float tri_norm3(const float *v) { return fsqrt(dot3(v[0], v[1], v[2], v[0], v[1], v[2])); }

// The right singular vector of A's least singular value (A row-major, float), in double: the one-sided Jacobi of
// vsg_jacobi.h on the columns of A, kTriSweeps sweeps, the matrix in registers (loops are compile-time bounded and the
// column is taken with selects).
VSG_HD void tri_null_vector(const float *A, double *v) {
  JacobiRegs<4, 4> s;
  for (int r = 0; r < 4; r++)
    for (int c = 0; c < 4; c++) s.at(r, c) = (double)A[4 * r + c], s.at(4 + r, c) = r == c ? 1.0 : 0.0;
  jacobi_sweeps<4, 4, kTriSweeps>(s);
  jacobi_null_vector<4, 4>(s, v);
}

// GeometricTools::Triangulate (GeometricTools.cc:47-66): false = x3Dh(3) == 0
VSG_HD bool tri_triangulate(const float *xn1, const float *xn2, const vsg_frame_pose &c1, const vsg_frame_pose &c2, float *x3D) {
  float A[16];
  for (int c = 0; c < 4; c++) {  // Tcw = [Rcw | tcw]: row r, column c
    const float t10 = c < 3 ? c1.Rcw[c] : c1.tcw[0], t11 = c < 3 ? c1.Rcw[3 + c] : c1.tcw[1], t12 = c < 3 ? c1.Rcw[6 + c] : c1.tcw[2];
    const float t20 = c < 3 ? c2.Rcw[c] : c2.tcw[0], t21 = c < 3 ? c2.Rcw[3 + c] : c2.tcw[1], t22 = c < 3 ? c2.Rcw[6 + c] : c2.tcw[2];
    A[c] = fsub(fmul(xn1[0], t12), t10);       // :50
    A[4 + c] = fsub(fmul(xn1[1], t12), t11);   // :51
    A[8 + c] = fsub(fmul(xn2[0], t22), t20);   // :52
    A[12 + c] = fsub(fmul(xn2[1], t22), t21);  // :53
  }
  double v[4];
  tri_null_vector(A, v);  // :55-57
  const float h0 = (float)v[0], h1 = (float)v[1], h2 = (float)v[2], h3 = (float)v[3];
  if (h3 == 0) return false;  // :59-60
  x3D[0] = fdiv(h0, h3), x3D[1] = fdiv(h1, h3), x3D[2] = fdiv(h2, h3);  // :63
  return true;
}

// KeyFrame::UnprojectStereo (KeyFrame.cc:885-902) given x3Dc: false = !(z > 0)
VSG_HD bool tri_unproject_stereo(const vsg_frame_pose &c, const float *xyz_c, float *x3D) {
  if (xyz_c[2] > 0) {
    float r[3];
    tri_rotate_wc(c, xyz_c, r);
    x3D[0] = fadd(r[0], c.Ow[0]), x3D[1] = fadd(r[1], c.Ow[1]), x3D[2] = fadd(r[2], c.Ow[2]);  // :897
    return true;
  }
  return false;
}

// one reprojection gate (:620-645 / :647-670): true = rejected.  mbf is ALWAYS the current keyframe's (:638 and :663)
VSG_HD bool tri_reprojection_rejects(const vsg_frame_pose &c, float mbf_current, const TriFeature &f, bool stereo, float xc,
                                     float yc, float zc) {
  const float invz = (float)ddiv(1.0, (double)zc);  // :624, :651: const float invz = 1.0 / z
  if (!stereo) {
    const float u = fadd(fdiv(fmul(c.fx, xc), zc), c.cx), v = fadd(fdiv(fmul(c.fy, yc), zc), c.cy);  // Pinhole.cpp:33-34
    const float ex = fsub(u, f.x), ey = fsub(v, f.y);
    return (double)fadd(fmul(ex, ex), fmul(ey, ey)) > dmul(5.991, (double)f.level_sigma2);  // :632 / :657
  }
  const float u = fadd(fmul(fmul(c.fx, xc), invz), c.cx);  // :637 / :662
  const float ur = fsub(u, fmul(mbf_current, invz));       // :638 / :663
  const float v = fadd(fmul(fmul(c.fy, yc), invz), c.cy);  // :639 / :664
  const float ex = fsub(u, f.x), ey = fsub(v, f.y), er = fsub(ur, f.uright);
  return (double)fadd(fadd(fmul(ex, ex), fmul(ey, ey)), fmul(er, er)) > dmul(7.8, (double)f.level_sigma2);  // :643 / :668
}

// :557-562: xn = unprojectEig(kp.pt), ray = Rwc * xn, cosParallaxRays = ray1.dot(ray2) / (ray1.norm() * ray2.norm())
VSG_HD float tri_cos_parallax_rays(const vsg_frame_pose &c1, const vsg_frame_pose &c2, const TriFeature &f1, const TriFeature &f2,
                                   float *xn1, float *xn2, float *ray1, float *ray2) {
  tri_unproject(c1, f1.x, f1.y, xn1);
  tri_unproject(c2, f2.x, f2.y, xn2);
  tri_rotate_wc(c1, xn1, ray1);
  tri_rotate_wc(c2, xn2, ray2);
  return fdiv(dot3(ray1[0], ray1[1], ray1[2], ray2[0], ray2[1], ray2[2]), fmul(tri_norm3(ray1), tri_norm3(ray2)));
}

// The pair.  f1 = the current keyframe's feature idx1, f2 = pKF2's feature idx2.
VSG_HD TriOut triangulate_pair(const vsg_triangulation_params &P, const TriFeature &f1, const TriFeature &f2) {
  TriOut o = {kTriAccepted, kTriFromTriangulate, {0.0f, 0.0f, 0.0f}};
  const vsg_frame_pose &c1 = P.kf1, &c2 = P.kf2;
  const bool bStereo1 = f1.uright >= 0, bStereo2 = f2.uright >= 0;  // :486, :495 (no mpCamera2)
  // ---- parallax between the rays (:557-562)
  float xn1[3], xn2[3], ray1[3], ray2[3];
  const float cosParallaxRays = tri_cos_parallax_rays(c1, c2, f1, f2, xn1, xn2, ray1, ray2);
  // ---- stereo parallax (:564-576): kf2's value is taken only when kf1's feature is mono (the else if)
  const float cosParallaxStereo0 = fadd(cosParallaxRays, 1.0f);
  float cosParallaxStereo1 = cosParallaxStereo0, cosParallaxStereo2 = cosParallaxStereo0;
  if (bStereo1)
    cosParallaxStereo1 = f1.cos_stereo;
  else if (bStereo2)
    cosParallaxStereo2 = f2.cos_stereo;
  const float cosParallaxStereo = cosParallaxStereo2 < cosParallaxStereo1 ? cosParallaxStereo2 : cosParallaxStereo1;  // std::min
  // ---- :582-603; the float is compared with the double literals
  bool good;
  if (cosParallaxRays < cosParallaxStereo && cosParallaxRays > 0 &&
      (bStereo1 || bStereo2 || ((double)cosParallaxRays < 0.9996 && P.inertial) ||
       ((double)cosParallaxRays < 0.9998 && !P.inertial))) {
    if (!tri_triangulate(xn1, xn2, c1, c2, o.x3D)) {
      o.reason = kTriWZero;
      return o;
    }
    good = true;
  } else if (bStereo1 && cosParallaxStereo1 < cosParallaxStereo2) {
    o.source = kTriFromStereo1;
    good = tri_unproject_stereo(c1, f1.xyz_c, o.x3D);
  } else if (bStereo2 && cosParallaxStereo2 < cosParallaxStereo1) {
    o.source = kTriFromStereo2;
    good = tri_unproject_stereo(c2, f2.xyz_c, o.x3D);
  } else {
    o.reason = kTriLowParallax;
    return o;
  }
  if (!good) {  // :608
    o.reason = kTriStereoDepth;
    return o;
  }
  // ---- in front of both cameras (:611-618)
  const float z1 = tri_camera_coord(c1, 2, o.x3D);
  if (z1 <= 0) {
    o.reason = kTriZ1;
    return o;
  }
  const float z2 = tri_camera_coord(c2, 2, o.x3D);
  if (z2 <= 0) {
    o.reason = kTriZ2;
    return o;
  }
  // ---- reprojection in the first keyframe, then the second (:620-670)
  if (tri_reprojection_rejects(c1, c1.mbf, f1, bStereo1, tri_camera_coord(c1, 0, o.x3D), tri_camera_coord(c1, 1, o.x3D), z1)) {
    o.reason = kTriReproj1;
    return o;
  }
  if (tri_reprojection_rejects(c2, c1.mbf, f2, bStereo2, tri_camera_coord(c2, 0, o.x3D), tri_camera_coord(c2, 1, o.x3D), z2)) {
    o.reason = kTriReproj2;
    return o;
  }
  // ---- scale consistency (:672-689)
  const float n1[3] = {fsub(o.x3D[0], c1.Ow[0]), fsub(o.x3D[1], c1.Ow[1]), fsub(o.x3D[2], c1.Ow[2])};
  const float n2[3] = {fsub(o.x3D[0], c2.Ow[0]), fsub(o.x3D[1], c2.Ow[1]), fsub(o.x3D[2], c2.Ow[2])};
  const float dist1 = tri_norm3(n1), dist2 = tri_norm3(n2);
  if (dist1 == 0 || dist2 == 0) {
    o.reason = kTriDistZero;
    return o;
  }
  if (P.far_points && (dist1 >= P.th_far_points || dist2 >= P.th_far_points)) {
    o.reason = kTriFar;
    return o;
  }
  const float ratioDist = fdiv(dist2, dist1), ratioOctave = fdiv(f1.scale_factor, f2.scale_factor);
  if (fmul(ratioDist, P.ratio_factor) < ratioOctave || ratioDist > fmul(ratioOctave, P.ratio_factor)) o.reason = kTriScaleRatio;
  return o;
}

// The new MapPoint's UpdateNormalAndDepth (:704): two observations in the std::map<KeyFrame *>'s order -- pKF2 first when
// kf2_first -- and mpRefKF = the current keyframe (:692), whose keypoint's octave and scale table give the depth range.
// The routine itself is vsg_observations.h's.
VSG_HD void new_point_normal_and_depth(const vsg_triangulation_params &P, const float *x3D, int octave1,
                                       const float *scale_factors1, int nlevels, float *normal, float *min_dist,
                                       float *max_dist) {
  const vsg_frame_pose &a = P.kf2_first ? P.kf2 : P.kf1, &b = P.kf2_first ? P.kf1 : P.kf2;
  const float Ow[6] = {a.Ow[0], a.Ow[1], a.Ow[2], b.Ow[0], b.Ow[1], b.Ow[2]};
  const int32_t kf[2] = {0, 1};
  update_normal_and_depth(x3D, 2, kf, Ow, P.kf2_first ? 1 : 0, octave1, scale_factors1, nlevels, normal, min_dist, max_dist);
}


// ---- the host's side of a call: what is refused before anything is enqueued, and the loop itself on one thread (the tests'
// host build and the latency probe's caller-side path run it; the device runs k_new_points of vsg_triangulate.hip)

// every match is "none" (< 0) or a feature of kf2: the kernel indexes kf2 with these
inline bool tri_matches_ok(int n1, int n2, const int32_t *matches12) {
  for (int i = 0; i < n1; i++)
    if (matches12[i] >= n2) return false;
  return true;
}
// every free slot lies in the store and is listed once; seen = capacity zeros, left dirty
inline bool tri_free_slots_ok(int capacity, const int32_t *free_slots, int n_free, uint8_t *seen) {
  if (n_free < 0 || (n_free > 0 && !free_slots)) return false;
  for (int k = 0; k < n_free; k++) {
    const int s = free_slots[k];
    if (s < 0 || s >= capacity || seen[s]) return false;
    seen[s] = 1;
  }
  return true;
}
template <class OctaveOf>
inline bool tri_octaves_ok(int n, OctaveOf octave_of, int nlevels) {
  for (int i = 0; i < n; i++)
    if (octave_of(i) < 0 || octave_of(i) >= nlevels) return false;
  return true;
}

// one keyframe as the loop reads it; stereo = {x3Dc, cos parallax} per feature (4 floats), nullptr: no stereo keypoint
struct TriFrameHost {
  int n;
  const float *x, *y;
  const int32_t *octave;
  const float *uright;  // nullptr: every mvuRight is -1
  const float *stereo;
  const uint8_t *desc;
  const float *scale_factors, *level_sigma2;
};
inline TriFeature tri_feature_host(const TriFrameHost &F, int i) {
  TriFeature f;
  f.x = F.x[i], f.y = F.y[i], f.uright = F.uright ? F.uright[i] : -1.0f;
  f.scale_factor = F.scale_factors[F.octave[i]], f.level_sigma2 = F.level_sigma2[F.octave[i]];
  f.cos_stereo = 0.0f, f.xyz_c[0] = f.xyz_c[1] = f.xyz_c[2] = 0.0f;
  if (f.uright >= 0 && F.stereo) {
    const float *s = F.stereo + 4 * (size_t)i;
    f.xyz_c[0] = s[0], f.xyz_c[1] = s[1], f.xyz_c[2] = s[2], f.cos_stereo = s[3];
  }
  return f;
}
// a store's arrays on the host (pos == nullptr: geometry only)
struct TriStoreHost {
  float *pos, *normal, *min_dist, *max_dist;
  uint8_t *desc, *observed;
};
// The loop :475-708 in ascending idx1.  Outputs as vsg_frame_triangulate_matches; returns the number of points created.
inline int new_points_loop(const vsg_triangulation_params &P, const TriFrameHost &A, const TriFrameHost &B,
                           const int32_t *matches12, int nlevels, const TriStoreHost &S, const int32_t *free_slots, int n_free,
                           uint8_t *reason, uint8_t *source, float *x3d, int32_t *new_slot) {
  int created = 0;
  for (int i = 0; i < A.n; i++) {
    const int m = matches12[i];
    TriOut o = {kTriNoMatch, kTriFromTriangulate, {0.0f, 0.0f, 0.0f}};
    int slot = -1;
    if (m >= 0) {
      o = triangulate_pair(P, tri_feature_host(A, i), tri_feature_host(B, m));
      if (o.reason == kTriAccepted && S.pos) {
        if (created < n_free) {
          slot = free_slots[created++];
          const size_t s = (size_t)slot;
          for (int k = 0; k < 3; k++) S.pos[3 * s + k] = o.x3D[k];
          const uint8_t *row = P.kf2_first ? B.desc + 32 * (size_t)m : A.desc + 32 * (size_t)i;
          for (int k = 0; k < 32; k++) S.desc[32 * s + k] = row[k];
          new_point_normal_and_depth(P, o.x3D, A.octave[i], A.scale_factors, nlevels, S.normal + 3 * s, S.min_dist + s,
                                     S.max_dist + s);
          S.observed[s] = 1;
        } else {
          o.reason = kTriNoFreeSlot;
        }
      }
    }
    reason[i] = (uint8_t)o.reason, source[i] = (uint8_t)o.source, new_slot[i] = slot;
    for (int k = 0; k < 3; k++) x3d[3 * (size_t)i + k] = o.x3D[k];
  }
  return created;
}

}  // namespace vsg
