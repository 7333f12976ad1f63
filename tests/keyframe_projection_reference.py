"""NumPy float32 restatement of the per-point loop the four back-end routines that project map points into ONE KeyFrame
share, the yardstick of vsg_frame_fuse_points / vsg_frame_fuse_points_sim3 / vsg_frame_search_sim3_points and of
vsg::project_keyframe_point (visual_sgraphs_amd/csrc/vsg_project.h):

  Fuse(pKF, vpMapPoints, th, bRight = false)                          ORBmatcher.cc:1194-1241
  Fuse(pKF, Scw, vpPoints, th, vpReplacePoint)                        ORBmatcher.cc:1360-1395
  SearchByProjection(pKF, Scw, vpPoints, vpMatched, th, ratioHamming) ORBmatcher.cc:452-486 (and its twin, :559-595)
  KeyFrame::IsInImage                                                 KeyFrame.cc:880-883
  KeyFrame::mnMinX .. mnMaxY (const int, from the Frame's floats)     KeyFrame.h:419-422, KeyFrame.cc:52

Written from those lines (the pose-form Fuse is the one that also needs invz and ur; the Sim3 routines decompose Scw into
Tcw / Ow on entry, :433-434 and :1340-1341, and run the same steps), in the fixed order the project pins
(tests/frustum_reference.py: left to right, one correctly rounded float32 operation each).  Two things differ from the
Frame-side restatements of tests/projection_reference.py: IsInImage excludes the maximum and REJECTS a NaN, and the
bounds are ints -- the Frame's floats truncated toward zero.

It also builds the arrays the existing Frame.Fuse / Fuse_Sim3 / SearchByProjection_Sim3 bindings take: compacted to the
projected points, in order, with the index map back to the queries."""
import numpy as np

from projection_reference import _camera_point, _dot3, _project, map_back, predict_scale  # noqa: F401  (re-exported)

F32 = np.float32
# `why` of a point: where it left the loop
PROJECTED, SKIPPED, BEHIND, OUTSIDE_IMAGE, OUTSIDE_DISTANCE, NORMAL = 0, 1, 2, 3, 4, 5


def keyframe_bounds(bounds):
    """(mnMinX, mnMinY, mnMaxX, mnMaxY) of the KeyFrame built from a Frame with these float bounds: `const int`
    members initialised from floats (KeyFrame.cc:52), i.e. truncated toward zero."""
    return tuple(int(F32(b)) for b in bounds)


def project_keyframe_points(pose, bounds, P, Pn, mf_min, mf_max, skip=None):
    """ORBmatcher.cc:1194-1238 for every point.  bounds = the FRAME's (mnMinX, mnMinY, mnMaxX, mnMaxY) as floats; the
    KeyFrame's truncated ones are derived here.  mf_min, mf_max = the members mfMinDistance / mfMaxDistance.  skip[i] != 0:
    the routine `continue`s before GetWorldPos().  Returns valid, u, v, ur, level (0 where not valid), why, z."""
    P = np.asarray(P, F32).reshape(-1, 3)
    Pn = np.asarray(Pn, F32).reshape(-1, 3)
    mf_min, mf_max = np.asarray(mf_min, F32).reshape(-1), np.asarray(mf_max, F32).reshape(-1)
    n = len(P)
    Ow = pose["Ow"]
    minX, minY, maxX, maxY = (F32(b) for b in keyframe_bounds(bounds))  # int -> float in the comparisons of IsInImage
    with np.errstate(all="ignore"):
        Pc = _camera_point(pose, P)                                        # :1195
        z = Pc[2]
        invz = (F32(1.0) / z).astype(F32)                                  # :1204
        u, v = _project(pose, Pc)                                          # :1206
        ur = (u - (pose["mbf"] * invz).astype(F32)).astype(F32)            # :1215
        PO = [(P[:, i] - Ow[i]).astype(F32) for i in range(3)]             # :1219
        dist = np.sqrt(_dot3(PO[0], PO[1], PO[2], PO[0], PO[1], PO[2])).astype(F32)      # :1220
        max_d, min_d = (F32(1.2) * mf_max).astype(F32), (F32(0.8) * mf_min).astype(F32)  # MapPoint.cc:521-531
        dot = _dot3(PO[0], PO[1], PO[2], Pn[:, 0], Pn[:, 1], Pn[:, 2])     # PO.dot(Pn): float
        half = np.float64(0.5) * dist.astype(np.float64)                   # 0.5 * dist3D: double
    assert all(a.dtype == F32 for a in (invz, u, v, ur, dist, max_d, min_d, dot)) and half.dtype == np.float64
    out = dict(valid=np.zeros(n, np.uint8), u=np.zeros(n, F32), v=np.zeros(n, F32), ur=np.zeros(n, F32),
               level=np.zeros(n, np.int32), why=np.zeros(n, np.int32), z=z)
    for i in range(n):
        if skip is not None and skip[i]:
            out["why"][i] = SKIPPED
            continue
        if z[i] < F32(0.0):                                                # :1198 (0 and NaN go on)
            out["why"][i] = BEHIND
            continue
        if not (u[i] >= minX and u[i] < maxX and v[i] >= minY and v[i] < maxY):  # :1209, KeyFrame.cc:882 (a NaN fails)
            out["why"][i] = OUTSIDE_IMAGE
            continue
        if dist[i] < min_d[i] or dist[i] > max_d[i]:                       # :1223
            out["why"][i] = OUTSIDE_DISTANCE
            continue
        if np.float64(dot[i]) < half[i]:                                   # :1232
            out["why"][i] = NORMAL
            continue
        out["valid"][i], out["u"][i], out["v"][i], out["ur"][i] = 1, u[i], v[i], ur[i]
        out["level"][i] = predict_scale(mf_max[i], dist[i], pose["log_scale_factor"], pose["n_levels"])  # :1238
    return out


def check_scene(ref):
    """The condition a parity scene must meet, on the restatement alone: every reject branch removes at least one point and
    at least half of the points that are not skipped pass."""
    why = ref["why"]
    for k in (BEHIND, OUTSIDE_IMAGE, OUTSIDE_DISTANCE, NORMAL):
        assert (why == k).any(), k
    asked = int((why != SKIPPED).sum())
    assert 2 * int(ref["valid"].sum()) >= asked > 0, (int(ref["valid"].sum()), asked)


def fuse_fields(ref, slots, desc, th, scale_factors):
    """The arrays Frame.Fuse / Fuse_Sim3 / SearchByProjection_Sim3 take, compacted to the projected points in order;
    `index` maps an entry back to its query.  desc is per slot; radius = th * mvScaleFactors[nPredictedLevel] (:1241)."""
    idx = np.flatnonzero(ref["valid"])
    s = np.asarray(slots)[idx]
    lvl = ref["level"][idx]
    radius = (F32(th) * np.asarray(scale_factors, F32)[lvl]).astype(F32)
    return dict(index=idx, desc=np.ascontiguousarray(desc[s]).reshape(-1, 32), u=ref["u"][idx], v=ref["v"][idx],
                ur=ref["ur"][idx], radius=radius, predicted_level=lvl.astype(np.int32))


def spread(index, n, values, fill):
    """Per-entry results of a compacted call -> per query (fill where the query was not projected)."""
    out = np.full(n, fill, np.int32)
    out[index] = values
    return out
