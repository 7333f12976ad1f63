"""NumPy float32 restatement of the map-point side of Tracking::SearchLocalPoints, the yardstick of the resident
map-point path (vsg_mappoints_*, vsg_frame_is_in_frustum, vsg_frame_search_local_points):

  Frame::isInFrustum (Nleft == -1)   mbTrackInView, mTrackProjX/Y/XR, mTrackDepth, ...     Frame.cc:656-719
  Pinhole::project                   fx * X / Z + cx                                       CameraModels/Pinhole.cpp:46-53
  MapPoint::GetMin/MaxDistanceInvariance   0.8f * mfMinDistance, 1.2f * mfMaxDistance      MapPoint.cc:521-531
  MapPoint::PredictScale             ceil(log(mfMaxDistance / dist) / mfLogScaleFactor)    MapPoint.cc:550-565
  ORBmatcher::RadiusByViewingCos     the window of SearchByProjection(F, vpMapPoints)      ORBmatcher.cc:218-224, 59-70

Written from those lines.  The reference computes in Eigen float under -O3 -march=native, where the compiler decides
which products contract; this restatement fixes the order the project pins (left to right, one correctly rounded
float32 operation each: NumPy never contracts): dot products as ((a0 b0 + a1 b1) + a2 b2), norms as sqrtf of that,
u = (fx X) / Z + cx.  log is glibc's logf through ctypes -- np.log on float32 is NumPy's own SIMD routine.  PredictScale
divides the MEMBER mfMaxDistance, while the distance band uses the getters' scaled values; both are taken from the
members here, as the reference does."""
import ctypes as C
import ctypes.util

import numpy as np

F32 = np.float32
_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.logf.restype = C.c_float
_libm.logf.argtypes = [C.c_float]

NOT_SKIPPED, BEHIND, OUTSIDE_IMAGE, OUTSIDE_DISTANCE, VIEW_COS, SKIPPED = 0, 1, 2, 3, 4, 5  # `why` of a point


def logf(x):
    return F32(_libm.logf(float(F32(x))))


def cvt_int_x86(f):
    """(int)f of an x86-64 build (cvttss2si): truncation; NaN and anything outside [-2^31, 2^31) give INT_MIN."""
    f = float(f)
    if f != f or f < -2147483648.0 or f >= 2147483648.0:
        return -2147483648
    return int(f)


def predict_scale(mf_max_distance, dist, log_scale_factor, n_levels):
    """MapPoint::PredictScale (MapPoint.cc:550-565)."""
    with np.errstate(all="ignore"):
        ratio = F32(mf_max_distance) / F32(dist)
        n_scale = cvt_int_x86(np.ceil(F32(logf(ratio) / F32(log_scale_factor))))
    if n_scale < 0:
        n_scale = 0
    elif n_scale >= n_levels:
        n_scale = n_levels - 1
    return n_scale


def make_pose(Rcw, tcw, fx, fy, cx, cy, mbf, scale_factor=1.2, n_levels=8, Ow=None):
    """The camera of a Frame.  mOw = Twc.translation() (Frame::UpdatePoseMatrices, Frame.cc:612-619): passed by the caller of
    the library; here -Rcw^T tcw rounded from double when not given.  mfLogScaleFactor = log(mfScaleFactor) in float
    (ORBextractor::GetScaleFactor is a float, Frame.cc:113)."""
    R = np.asarray(Rcw, F32).reshape(3, 3)
    t = np.asarray(tcw, F32).reshape(3)
    if Ow is None:
        Ow = (-(R.T.astype(np.float64) @ t.astype(np.float64))).astype(F32)
    return dict(Rcw=R, tcw=t, Ow=np.asarray(Ow, F32).reshape(3), fx=F32(fx), fy=F32(fy), cx=F32(cx), cy=F32(cy),
                mbf=F32(mbf), log_scale_factor=logf(F32(scale_factor)), n_levels=int(n_levels))


def _dot3(a0, a1, a2, b0, b1, b2):
    return ((a0 * b0 + a1 * b1) + a2 * b2).astype(F32)


def is_in_frustum(pose, bounds, P, Pn, mf_min, mf_max, viewing_cos_limit=0.5, skip=None):
    """Frame::isInFrustum for every map point.  bounds = (mnMinX, mnMinY, mnMaxX, mnMaxY); P, Pn = GetWorldPos(),
    GetNormal(); mf_min, mf_max = the members mfMinDistance, mfMaxDistance.  skip: points Tracking::SearchLocalPoints never
    projects (Tracking.cc:3450-3453).  Returns a dict of per-point arrays; `why` says where a point left."""
    P = np.asarray(P, F32).reshape(-1, 3)
    Pn = np.asarray(Pn, F32).reshape(-1, 3)
    mf_min, mf_max = np.asarray(mf_min, F32).reshape(-1), np.asarray(mf_max, F32).reshape(-1)
    n = len(P)
    R, t, Ow = pose["Rcw"], pose["tcw"], pose["Ow"]
    minX, minY, maxX, maxY = (F32(b) for b in bounds)
    lim = F32(viewing_cos_limit)
    with np.errstate(all="ignore"):
        Pc = [(_dot3(R[i, 0], R[i, 1], R[i, 2], P[:, 0], P[:, 1], P[:, 2]) + t[i]).astype(F32) for i in range(3)]  # :668
        Pc_dist = np.sqrt(_dot3(Pc[0], Pc[1], Pc[2], Pc[0], Pc[1], Pc[2])).astype(F32)                              # :669
        z = Pc[2]
        invz = (F32(1.0) / z).astype(F32)                                                                           # :673
        u = ((pose["fx"] * Pc[0]).astype(F32) / z + pose["cx"]).astype(F32)                                         # Pinhole.cpp:49-50
        v = ((pose["fy"] * Pc[1]).astype(F32) / z + pose["cy"]).astype(F32)
        PO = [(P[:, i] - Ow[i]).astype(F32) for i in range(3)]                                                      # :690
        dist = np.sqrt(_dot3(PO[0], PO[1], PO[2], PO[0], PO[1], PO[2])).astype(F32)
        max_d, min_d = (F32(1.2) * mf_max).astype(F32), (F32(0.8) * mf_min).astype(F32)                             # MapPoint.cc:521-531
        view_cos = (_dot3(PO[0], PO[1], PO[2], Pn[:, 0], Pn[:, 1], Pn[:, 2]) / dist).astype(F32)                     # :699
        xr = (u - (pose["mbf"] * invz).astype(F32)).astype(F32)                                                     # :710
    assert all(a.dtype == F32 for a in (Pc_dist, u, v, dist, view_cos, xr, max_d, min_d))
    out = dict(in_view=np.zeros(n, np.uint8), proj_x=np.full(n, -1, F32), proj_y=np.full(n, -1, F32),
               proj_xr=np.zeros(n, F32), depth=np.zeros(n, F32), scale_level=np.zeros(n, np.int32),
               view_cos=np.zeros(n, F32), why=np.zeros(n, np.int32))
    for i in range(n):
        if skip is not None and skip[i]:
            out["why"][i] = SKIPPED
            continue
        if z[i] < F32(0.0):                                       # :674-675
            out["why"][i] = BEHIND
            continue
        if u[i] < minX or u[i] > maxX or v[i] < minY or v[i] > maxY:  # :679-682
            out["why"][i] = OUTSIDE_IMAGE
            continue
        out["proj_x"][i], out["proj_y"][i] = u[i], v[i]             # :684-685
        if dist[i] < min_d[i] or dist[i] > max_d[i]:                # :693-694
            out["why"][i] = OUTSIDE_DISTANCE
            continue
        if view_cos[i] < lim:                                       # :701-702
            out["why"][i] = VIEW_COS
            continue
        out["in_view"][i] = 1
        out["scale_level"][i] = predict_scale(mf_max[i], dist[i], pose["log_scale_factor"], pose["n_levels"])  # :705
        out["proj_xr"][i], out["depth"][i], out["view_cos"][i] = xr[i], Pc_dist[i], view_cos[i]
    return out


def search_fields(ref, desc, observed, th_far_points=None):
    """The per-map-point arrays vsg_frame_search_by_projection takes, from is_in_frustum's result: a point beyond
    thFarPoints (bFarPoints, ORBmatcher.cc:53-54) is handed over as not in view -- it is not searched."""
    in_view = ref["in_view"].copy()
    if th_far_points is not None:
        in_view[ref["depth"] > F32(th_far_points)] = 0
    return dict(desc=desc, observed=observed, in_view=in_view, proj_x=ref["proj_x"], proj_y=ref["proj_y"],
                proj_xr=ref["proj_xr"], scale_level=ref["scale_level"], view_cos=ref["view_cos"])


# ---- seeded scenarios
CAMERAS = {
    # name: (width, height, fx, fy, cx, cy, mbf)
    "tum1": (640, 480, 517.306408, 516.469215, 318.643040, 255.313989, 40.0),
    "euroc": (752, 480, 458.654, 457.296, 367.215, 248.375, 47.90639384423901),
    "hd720": (1280, 720, 912.0, 911.0, 637.5, 362.25, 45.6),
}


def rotation(rng, max_angle):
    """A rotation by up to max_angle about each axis (Z Y X), float32."""
    ax, ay, az = rng.uniform(-max_angle, max_angle, 3)
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return (Rz @ Ry @ Rx).astype(F32)


def scenario(seed, camera="tum1", n=4000, n_levels=8, scale_factor=1.2):
    """A local map around a camera within +-0.3 rad / +-0.5 m of the origin: n points in the box [-6,6] x [-4,4] x [-2,10],
    normals towards a jittered reference-keyframe centre with unit-scale angular noise, distance members from a random
    octave of the reference keyframe (MapPoint::UpdateNormalAndDepth, MapPoint.cc:505-510).  The octave is drawn one level
    wider than the pyramid on both sides so that the predicted level reaches 0 and n_levels - 1.  Returns (pose, bounds,
    fields) with fields = world_pos, normal, min_dist, max_dist (the members), desc, observed."""
    w, h, fx, fy, cx, cy, mbf = CAMERAS[camera]
    rng = np.random.default_rng(1000 + seed)
    pose = make_pose(rotation(rng, 0.3), rng.uniform(-0.5, 0.5, 3), fx, fy, cx, cy, mbf, scale_factor, n_levels)
    bounds = (0.0, 0.0, float(w), float(h))
    P = np.stack([rng.uniform(-6, 6, n), rng.uniform(-4, 4, n), rng.uniform(-2, 10, n)], 1).astype(F32)
    ref = rng.normal(0, 1.5, (n, 3)).astype(F32)
    d0 = np.linalg.norm((P - ref).astype(np.float64), axis=1)
    Nn = (P - ref).astype(np.float64) + rng.normal(0, 1.0, (n, 3)) * d0[:, None]
    Nn = (Nn / np.linalg.norm(Nn, axis=1, keepdims=True)).astype(F32)
    lvl = rng.integers(-1, n_levels + 1, n)
    sf = F32(scale_factor)
    mf_max = (d0.astype(F32) * sf ** lvl.astype(F32)).astype(F32)           # dist * levelScaleFactor
    mf_min = (mf_max / sf ** F32(n_levels - 1)).astype(F32)                  # / mvScaleFactors[nLevels - 1]
    fields = dict(world_pos=P, normal=Nn, min_dist=mf_min, max_dist=mf_max,
                  desc=rng.integers(0, 256, (n, 32), dtype=np.uint8), observed=(rng.random(n) < 0.8).astype(np.uint8))
    return pose, bounds, fields


def scenario_shares(ref):
    """Shares of the points by `why`, and the distinct predicted levels among the in-view ones."""
    why = ref["why"]
    shares = {k: float((why == k).mean()) for k in (NOT_SKIPPED, BEHIND, OUTSIDE_IMAGE, OUTSIDE_DISTANCE, VIEW_COS)}
    return shares, sorted(set(ref["scale_level"][ref["in_view"] != 0].tolist()))


def check_scenario(ref):
    """The conditions every parity scenario must meet BEFORE the GPU is asked anything: in view >= 10 %, each of the four
    rejections >= 2 %, at least 6 distinct predicted levels among the in-view points."""
    shares, levels = scenario_shares(ref)
    assert shares[NOT_SKIPPED] >= 0.10, shares
    for k in (BEHIND, OUTSIDE_IMAGE, OUTSIDE_DISTANCE, VIEW_COS):
        assert shares[k] >= 0.02, (k, shares)
    assert len(levels) >= 6, levels
    return shares, levels
