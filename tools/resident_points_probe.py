#!/usr/bin/env python3
"""Warm latency of the searches on device-resident map points, next to what a caller does without them.  Runs on the GPU
box; every run is a fresh child process, the variants alternating call by call inside it.  Three cases, each a resident
1000-feature frame (640x480, TUM1 intrinsics) whose features sit where a subset of the points projects, with slightly
changed descriptors, so that the search matches a real share:

  local     Tracking::SearchLocalPoints, local maps of 1000 / 2000 / 4000 points (tests/frustum_reference.py's scenario)
            A = Frame::isInFrustum per point on the host + vsg_frame_search_by_projection
            B = vsg_frame_search_local_points;  B5 = B with 5 % of the slots updated before each call: a keyframe's churn
  last      SearchByProjection(CurrentFrame, LastFrame, th, bMono), last frames whose features carry 500 / 1000 / 2000
            slots (a quarter more features carry none)
            A = the projection loop of ORBmatcher.cc:1686-1715 on the host + vsg_frame_search_by_projection_last
            B = vsg_frame_search_last_frame, last frame and store resident
  keyframe  Fuse(pKF, vpMapPoints, th), 500 / 1000 / 2000 candidate points, a tenth flagged isBad() / IsInKeyFrame(pKF)
            A = the per-point loop of ORBmatcher.cc:1194-1241 on the host + vsg_frame_fuse
            B = vsg_frame_fuse_points (LocalMapping::SearchInNeighbors fuses one list into 20-30 neighbours, one pose each)
  refresh   MapPoint::ComputeDistinctiveDescriptors + UpdateNormalAndDepth of 500 / 2000 / 8000 points (a keyframe's
            points, a local and a large bundle adjustment's) observed in 30 resident keyframes of 1000 features
            A  = gather of the descriptors + both routines' loops on the host + vsg_mappoints_update of the four fields
            Ap = A with the descriptor choice by vsg_distinctive_descriptors;  B = vsg_mappoints_refresh_from_observations
  pose      Optimizer::PoseOptimization of a 1000-feature frame with 100 / 300 / 1000 correspondences (20 % outliers,
            half of the features stereo, the start pose a constant-velocity guess 2 cm and 1 degree off)
            A  = the host build of csrc/vsg_pose_opt.h on one thread, given the same arrays: the caller-side path as far as
                 it can be built here.  It is NOT g2o (no Eigen here) and likely flatters the host: same arithmetic, no
                 virtual calls, no sparse block solver.  B = vsg_frame_pose_optimization;  B2 = B again, the device
                 call's own A-vs-A repeat.  Every call asserts A and B equal bit for bit (pose, chi2, flags)

A is the caller-side path: the host loop (tools/resident_points_cpu.cpp, the kernel's own arithmetic compiled -O2, one
thread) + the gather of descriptors + the host-array entry point; A2 is A again, the run's own A-vs-A spread.  For B only
the pose changes (a small rotation per call, the same for every variant).  Host clock around the blocking calls, straight
through ctypes with preallocated arrays on both sides.  Every call asserts that A and B compute the same result.

  newpoints one neighbour of LocalMapping::CreateNewMapPoints on two resident keyframes of 1000 / 2000 features, a store of 8000
            slots, resident FeatureVectors
            A  = vsg_frame_search_for_triangulation_epipolar + the host build of csrc/vsg_triangulate.h over its matches on one
                 thread (NOT Eigen: the header's own arithmetic) + vsg_mappoints_update + vsg_mappoints_refresh_from_observations
            B  = vsg_frame_create_new_map_points;  A2 / B2 = both again.  Every call asserts equal outputs and store

  sim3      Sim3Solver on resident map points (LoopClosing.cc:678-690): 30 / 100 / 300 correspondences between two stores of 4096
            slots, 300 hypotheses, min_inliers 15; "loop" = a true loop (30 % outliers: the solver converges within the first few
            hypotheses), "false" = a false candidate (no consistent similarity: all 300 are walked)
            A  = vsg_mappoints_read of both point sets + the host build of csrc/vsg_sim3.h on one thread WITH the reference's
                 early exit (NOT Eigen: the header's own arithmetic)
            B  = vsg_mappoints_sim3_ransac (every hypothesis, no early exit);  A2 / B2 = both again.  Equal results asserted

  mlpnp     MLPnPsolver on a resident 1000-feature frame and a store of 4096 slots (Tracking::Relocalization, Tracking.cc:3735-3762):
            30 / 100 / 300 correspondences, SetRansacParameters(0.99, 10, 300, 6, 0.5, 5.991), the first iterate(5, ...); "true" = a
            true candidate (30 % outliers: the reference returns after a handful of hypotheses), "false" = a false one (every
            correspondence an outlier: all of mRansacMaxIts are walked)
            A  = vsg_mappoints_read + the host build of csrc/vsg_mlpnp.h on one thread WITH the reference's early return and
                 WITH Refine()'s solve over the best set, whose result the reference drops (NOT Eigen: the header's own Jacobi
                 and LDL^T)
            B  = vsg_frame_mlpnp_ransac (every hypothesis, no early return, no dropped solve);  A2 / B2 = both again.  Equal
                 results asserted on every call

  twoview   TwoViewReconstruction::Reconstruct (Tracking.cc:2568): 100 / 300 / 1000 matches between two frames of 1000 / 1000 /
            2000 features, 200 sets.  A = the host build of csrc/vsg_two_view.h on one thread, given the keypoint arrays (NOT
            Eigen), AT = the same with H and F on two threads as the reference runs them, B = vsg_frame_two_view_reconstruct;
            A2 / B2 = both again.  Equal results asserted on every call
  sim3opt   Optimizer::OptimizeSim3 on two resident keyframes of 1000 features (LoopClosing.cc:538, :747): 30 / 100 / 300 pairs
            between two stores of 4096 slots, 20 % outliers, th2 = 10, fix_scale 0 and 1 (a size is "<pairs>:<fix_scale>")
            A  = vsg_mappoints_read of both point sets + the host build of csrc/vsg_sim3_opt.h on one thread (NOT g2o: the
                 header's own arithmetic, numeric Jacobian included)
            B  = vsg_frame_optimize_sim3;  A2 / B2 = both again.  Every call asserts A and B equal bit for bit

  localba   the visual part of Optimizer::LocalBundleAdjustment on 10 + 10 / 20 + 20 / 40 + 40 optimised + fixed resident
            keyframes of 1000 features with 1500 / 3000 / 6000 points of 6 observations, half stereo, 5 % outliers, the start
            1 cm / 0.5 degrees off (a size is "<optimised = fixed keyframes>:<points>")
            A  = vsg_mappoints_read + the host build of csrc/vsg_local_ba.h on one thread (NOT g2o: the header's own
                 arithmetic and its DENSE reduced solve) + vsg_mappoints_update
            B  = vsg_mappoints_local_bundle_adjustment;  A2 / B2 = both again;  B_S1 / B_S2 / B_S10 = B with 1 / 2 / 10 trial
                 slots enqueued ahead per iteration instead of the library's.  Every call asserts all seven equal bit for bit

  sgraphba  Optimizer::LocalBundleAdjustment WITH its planes and rooms: the localba leg's scenes with 8 / 16 / 32 planes, each seen
            by a third of the keyframes, and 1 / 2 / 4 rooms (the first of four walls, the others corridors); a size is
            "<optimised = fixed keyframes>:<points>:<0 = the default factors, plane_point alone | 1 = plane_kf too>"
            A  = vsg_mappoints_read + the host build of csrc/vsg_sgraph_ba.h on one thread (NOT g2o: the header's own
                 arithmetic, numeric Jacobians and DENSE reduced solve included) + vsg_mappoints_update
            B  = vsg_mappoints_local_bundle_adjustment_sgraph;  A2 / B2 = both again;  V / V2 = the VISUAL call on the same
                 scene without its planes and rooms: B - V is the price of the semantic part.  Every call asserts A, B, A2
                 and B2 equal bit for bit
            `sgraphba trace [size]` runs one size five times, for rocprofv3 --kernel-trace --stats with VSG_NO_OVERLAP=1

  globalba  the visual part of Optimizer::BundleAdjustment behind GlobalBundleAdjustemnt: "init" = 1 fixed + 1 optimised
            keyframe, 300 mono points, robust, 20 iterations (CreateInitialMapMonocular); "50" / "100" / "200" / "500" = that many
            keyframes, one of them fixed, 15 points per keyframe of 8 observations (120 observed features per keyframe), half
            stereo, not robust, 10 iterations, write_store = 1 (RunGlobalBundleAdjustment).  Calls per size: 200 / 50 / 20 / 5 / 3
            (the host side takes seconds per call at the last two)
            A  = vsg_mappoints_read + the host build of csrc/vsg_global_ba.h on one thread (NOT g2o: the header's own
                 arithmetic and its DENSE reduced solve) + vsg_mappoints_update
            B  = vsg_mappoints_global_bundle_adjustment;  A2 / B2 = both again.  Every call asserts all four equal bit for bit
            `child globalba <calls> <size,size>` runs the listed sizes alone; `globalba trace [size]` runs the 100-keyframe problem
            (or the given size) through the new call and, up to 129 keyframes, through the local call, for rocprofv3 --kernel-trace --stats with VSG_NO_OVERLAP=1

  essgraph  Optimizer::OptimizeEssentialGraph (the pose graph of loop closing) on resident map points: 50 / 200 / 438 keyframes, one
            fixed, about 6 edges per keyframe and one loop edge, 10 map points per keyframe, fix_scale 0 and 1 (a size is
            "<keyframes>:<fix_scale>"), 3 iterations.  Calls per size: 200 / 50 / 5
            A  = vsg_mappoints_read + the host build of csrc/vsg_essential_graph.h on one thread (NOT g2o: the header's own
                 arithmetic, numeric Jacobian and DENSE solve included) + vsg_mappoints_update
            B  = vsg_mappoints_optimize_essential_graph;  A2 / B2 = both again.  Every call asserts all four equal bit for bit
            `essgraph trace [size]` runs the 200-keyframe problem three times, for rocprofv3 --kernel-trace --stats with VSG_NO_OVERLAP=1

  track / track_local   Tracking's two per-frame steps as chain calls (vsg_frame_track_with_motion_model,
            vsg_frame_track_local_map), 1000 / 2000 / 4000 points, against the caller-side path on the SAME library: the two
            existing calls plus the caller's loops on one thread.  A2 / B2 = both again; the walk's rounds where the result
            carries them.  Both write into profiles/track_chain_latency.json, one key each

usage: resident_points_probe.py <local|last|keyframe|refresh|pose|newpoints|sim3|mlpnp|sim3opt|localba|sgraphba|globalba|essgraph|twoview|track|track_local> [calls] [out.json]  -> runs the child, writes the record (default
                                  profiles/local_points_latency.json, track_last_latency.json, keyframe_points_latency.json,
                                  mappoints_refresh_latency.json, pose_optimization_latency.json)
       resident_points_probe.py child <case> [calls]  -> one JSON object on stdout (medians, 10-90 % range, microseconds)
       resident_points_probe.py local trace           -> a few B calls at 4000 points, for rocprofv3 --kernel-trace --stats
       resident_points_probe.py refresh trace         -> the same for refresh at 8000 points"""
import ctypes as C
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

_f32p, _u8p, _i32p = (C.POINTER(t) for t in (C.c_float, C.c_uint8, C.c_int32))
NFEAT = 1000
FIELDS = ("world_pos", "normal", "min_dist", "max_dist", "desc", "observed")


def host_side(orb):
    out = ROOT / "tools" / "_bin"
    out.mkdir(exist_ok=True)
    so = out / "libresident_points_cpu.so"
    csrc = ROOT / "visual_sgraphs_amd" / "csrc"
    src = [ROOT / "tools" / "resident_points_cpu.cpp", csrc / "vsg_project.h", csrc / "vsg_frustum.h", csrc / "vsg_math.h",
           csrc / "vsg_observations.h", csrc / "vsg_pose_opt.h", csrc / "vsg_triangulate.h", csrc / "vsg_sim3.h",
           csrc / "vsg_sim3_opt.h", csrc / "vsg_local_ba.h", csrc / "vsg_global_ba.h", csrc / "vsg_two_view.h", csrc / "vsg_jacobi.h", csrc / "vsg_mlpnp.h", csrc / "vsg_essential_graph.h",
           csrc / "vsg_sgraph_ba.h"]
    if not so.exists() or any(f.stat().st_mtime > so.stat().st_mtime for f in src):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-pthread", "-I", str(csrc), "-o",
                               str(so), str(src[0])])
    H = C.CDLL(str(so))
    pose = C.POINTER(orb.FramePose)
    H.lp_host_side.restype = None
    H.lp_host_side.argtypes = [pose, _f32p, C.c_float, C.c_int, _i32p, _f32p, _f32p, _f32p, _f32p, _u8p, _u8p, _u8p, _f32p,
                               _f32p, _f32p, _i32p, _f32p, _u8p, _u8p]
    H.tl_host_side.argtypes = [pose, _f32p, C.c_int, _i32p, C.c_void_p, _f32p, _u8p, _u8p, _i32p, _u8p, _u8p, _f32p, _f32p,
                               _f32p, _i32p, _f32p]
    H.kp_host_side.argtypes = [pose, _f32p, C.c_int, _u8p, _f32p, _f32p, _f32p, _f32p, _u8p, C.c_float, _f32p, _i32p, _u8p,
                               _f32p, _f32p, _f32p, _f32p, _i32p]
    H.rf_host_side.restype = H.rf_take_rows.restype = None
    H.rf_host_side.argtypes = [C.c_int, _i32p, _i32p, _i32p, _i32p, _u8p, _i32p, C.c_int, _f32p, _f32p, _f32p, C.c_int, C.c_int,
                               _u8p, _i32p, _u8p, _f32p, _f32p, _f32p]
    H.rf_take_rows.argtypes = [C.c_int, _i32p, _u8p, _i32p, _u8p]
    H.np_host_side.argtypes = [C.c_void_p, C.c_int, C.c_void_p, _i32p, C.c_int, C.c_void_p, _i32p, _i32p, C.c_int, _i32p, C.c_int,
                               _u8p, _u8p, _f32p, _i32p, _i32p, _f32p, _i32p]
    H.s3_host_side.argtypes = [C.c_int, _f32p, _f32p, _f32p, _f32p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, _i32p, _u8p,
                               C.c_void_p]
    H.so_host_side.argtypes = [C.c_int, C.c_int, _i32p, _i32p, _i32p, _i32p, C.c_int, C.c_int, _f32p, _f32p, _f32p, _f32p, _i32p,
                               _f32p, _f32p, _i32p, C.c_void_p, C.c_void_p, _f32p, _f32p, C.c_int, C.c_void_p, C.c_float, C.c_int,
                               C.c_int, _u8p, C.POINTER(C.c_double), C.c_void_p]
    H.lb_host_side.argtypes = [C.c_int, C.c_int, _i32p, _f32p, _i32p, _i32p, _i32p, C.c_int, _i32p, _f32p, _f32p, _i32p, _f32p,
                               C.c_void_p, _u8p, C.c_void_p, _f32p, C.c_int, C.c_int, C.c_void_p, _f32p, _u8p,
                               C.POINTER(C.c_double), C.c_void_p]
    f64p = C.POINTER(C.c_double)
    H.sg_host_side.argtypes = H.lb_host_side.argtypes[:-1] + [C.c_int, f64p, _i32p, _i32p, f64p, f64p, f64p, f64p, C.c_int, f64p, _i32p,
                                                              _i32p, f64p, f64p, _u8p, f64p, f64p, C.c_void_p]
    H.gb_host_side.argtypes = [C.c_int, C.c_int, _i32p, _f32p, _i32p, _i32p, _i32p, C.c_int, _i32p, _f32p, _f32p, _i32p, _f32p,
                               C.c_void_p, _u8p, C.c_void_p, _f32p, C.c_int, C.c_int, C.c_int, C.c_void_p, _f32p, _u8p,
                               C.POINTER(C.c_double), C.c_void_p]
    H.eg_host_side.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, _u8p, _u8p, C.c_int, _i32p, _i32p, _u8p, C.c_int, C.c_int,
                               C.c_int, _i32p, _i32p, _f32p, C.c_void_p, _f32p, C.POINTER(C.c_double), C.c_void_p]
    H.ml_host_side.argtypes = [C.c_int, _i32p, _f32p, _f32p, _f32p, _i32p, _f32p, _f32p, C.c_float, C.c_int, C.c_int, C.c_int, _i32p,
                               _u8p, C.c_void_p]
    H.tv_host_side.argtypes = [_f32p, C.c_int, _f32p, C.c_int, _i32p, _f32p, C.c_void_p, C.c_int, _i32p, C.c_int, C.c_void_p, _u8p, _f32p]
    H.tk_slots_from_matches.restype = H.tk_blocked_from_slots.restype = None
    H.tk_slots_from_matches.argtypes = [C.c_int, _i32p, _i32p, _i32p, _i32p]
    H.tk_blocked_from_slots.argtypes = [C.c_int, _i32p, _u8p, _u8p]
    H.tk_discard.argtypes = [C.c_int, C.c_int, _i32p, _u8p, _u8p, _i32p]
    H.tk_local_stats.argtypes = [C.c_int, _i32p, _u8p, _u8p, C.c_int, C.c_int]
    H.po_host_side.argtypes = [C.c_int, _i32p, _f32p, _f32p, _f32p, _i32p, _f32p, _f32p, _f32p, _f32p, C.c_int, _u8p, _f32p,
                               C.POINTER(C.c_double), _i32p]
    return H


def p(a, t):
    return a.ctypes.data_as(t)


def stats(us):
    a = np.sort(np.asarray(us))
    return {"median_us": round(float(np.median(a)), 1), "p10_us": round(float(a[int(0.1 * len(a))]), 1),
            "p90_us": round(float(a[int(0.9 * len(a))]), 1)}


class Case:
    """What the three cases share.  A case provides SIZES, TH, DEST, its scene (__init__(orb, fr, n): self.pose and
    self.bounds first), A(L, H, P) and B(L, P) -> the result to compare (computed inside the clock), and facts()."""
    VARIANTS = ("A", "B", "A2")

    def start(self, orb, fr, n):
        self.orb, self.fr, self.n = orb, fr, n
        self.sf = (np.float32(1.2) ** np.arange(8, dtype=np.float32)).astype(np.float32)
        self.b = np.array(self.bounds, np.float32)
        return np.random.default_rng(n)

    def cloud(self, rng):
        """n points in front of the camera, a tenth of them outside the image: (px, py) and self.pos"""
        po, n = self.pose, self.n
        R, t = po["Rcw"].astype(np.float64), po["tcw"].astype(np.float64)
        px, py, z = rng.uniform(-40, 680, n), rng.uniform(-30, 510, n), rng.uniform(1, 8, n)
        Pc = np.stack([(px - po["cx"]) / po["fx"] * z, (py - po["cy"]) / po["fy"] * z, z], 1)
        self.pos = np.ascontiguousarray(((Pc - t) @ R).astype(np.float32))
        return px, py

    def frame(self, x, y, octave, desc, rng, angle=False):
        """The resident frame: NFEAT features at (x, y) with two changed descriptor bytes each"""
        keys = np.zeros(NFEAT, self.orb.KP_DTYPE)
        keys["x"], keys["y"], keys["octave"] = x, y, octave
        if angle:
            keys["angle"] = rng.uniform(0, 360, NFEAT)
        d = desc.copy()
        d[:, :2] ^= rng.integers(0, 256, (NFEAT, 2), dtype=np.uint8)
        self.F = self.orb.Frame(NFEAT + 1)
        self.F.upload(keys, d, self.bounds)

    def pose_at(self, k):
        """The camera turned by a small angle about its y axis: the pose of call k."""
        a = 0.002 * (k % 50)
        Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        po = self.pose
        R = (Ry @ po["Rcw"].astype(np.float64)).astype(np.float32)
        t = (Ry @ po["tcw"].astype(np.float64)).astype(np.float32)
        return self.orb.FramePose.make(**self.fr.make_pose(R, t, po["fx"], po["fy"], po["cx"], po["cy"], po["mbf"]))

    def reset(self):
        pass

    def run(self, name, L, H, P):
        return self.A(L, H, P) if name[0] == "A" else self.B(L, P)


class Local(Case):
    SIZES, TH, NNRATIO, DEST = (1000, 2000, 4000), 3.0, 0.8, "local_points_latency.json"
    VARIANTS = ("A", "B", "A2", "B5")

    def __init__(self, orb, fr, n):
        self.pose, self.bounds, f = fr.scenario(3, "tum1", n=n)
        rng = self.start(orb, fr, n)
        self.f = {k: np.ascontiguousarray(v) for k, v in f.items()}
        ref = fr.is_in_frustum(self.pose, self.bounds, f["world_pos"], f["normal"], f["min_dist"], f["max_dist"])
        iv = np.flatnonzero(ref["in_view"])
        src = self.src = iv[rng.integers(0, len(iv), NFEAT)]
        x = ref["proj_x"][src] + rng.normal(0, 2.0, NFEAT).astype(np.float32)
        y = ref["proj_y"][src] + rng.normal(0, 2.0, NFEAT).astype(np.float32)
        self.frame(x, y, np.maximum(ref["scale_level"][src] - rng.integers(0, 2, NFEAT), 0), f["desc"][src], rng)
        self.mp = orb.MapPoints(n)
        self.slots = np.arange(n, dtype=np.int32)
        self.mp.update(self.slots, **{k: self.f[k] for k in FIELDS})
        z = np.zeros
        self.in_view, self.px, self.py, self.pxr = z(n, np.uint8), z(n, np.float32), z(n, np.float32), z(n, np.float32)
        self.lvl, self.vc, self.qd, self.qo = z(n, np.int32), z(n, np.float32), z((n, 32), np.uint8), z(n, np.uint8)
        self.tb, self.tm, self.ntm = z(NFEAT, np.uint8), z(NFEAT, np.int32), C.c_int(0)
        # the churn: 5 % of the slots rewritten with the values they hold
        self.churn = rng.choice(n, max(n // 20, 1), replace=False).astype(np.int32)
        self.u = [np.ascontiguousarray(self.f[k][self.churn]) for k in FIELDS[:5]]

    def reset(self):
        self.tb[:] = 0
        self.tm[:] = -1

    def A(self, L, H, P):
        f = self.f
        H.lp_host_side(C.byref(P), p(self.b, _f32p), 0.5, self.n, p(self.slots, _i32p), p(f["world_pos"], _f32p),
                       p(f["normal"], _f32p), p(f["min_dist"], _f32p), p(f["max_dist"], _f32p), p(f["desc"], _u8p),
                       p(f["observed"], _u8p), p(self.in_view, _u8p), p(self.px, _f32p), p(self.py, _f32p),
                       p(self.pxr, _f32p), p(self.lvl, _i32p), p(self.vc, _f32p), p(self.qd, _u8p), p(self.qo, _u8p))
        return L.vsg_frame_search_by_projection(
            self.F.handle, self.n, p(self.qd, _u8p), p(self.qo, _u8p), p(self.in_view, _u8p), p(self.px, _f32p),
            p(self.py, _f32p), p(self.pxr, _f32p), p(self.lvl, _i32p), p(self.vc, _f32p), None, None, None, None, None,
            self.TH, self.NNRATIO, p(self.sf, _f32p), 8, None, None, p(self.tb, _u8p), p(self.tm, _i32p))

    def B(self, L, P):
        return L.vsg_frame_search_local_points(
            self.F.handle, self.mp.handle, self.n, p(self.slots, _i32p), None, C.byref(P), 0.5, self.TH, self.NNRATIO, 0,
            0.0, p(self.sf, _f32p), 8, p(self.tb, _u8p), p(self.tm, _i32p), p(self.in_view, _u8p), p(self.px, _f32p),
            p(self.py, _f32p), C.byref(self.ntm))

    def run(self, name, L, H, P):
        if name == "B5":
            u = self.u
            assert L.vsg_mappoints_update(self.mp.handle, len(self.churn), p(self.churn, _i32p), p(u[0], _f32p),
                                          p(u[1], _f32p), p(u[2], _f32p), p(u[3], _f32p), p(u[4], _u8p), None) == 0
        return Case.run(self, name, L, H, P)

    def result(self, name, r):
        return r, self.tm.copy()

    def facts(self, last):
        return {"nmatches_last": int(last["B"][0]), "n_to_match_last": int(self.ntm.value)}


class Last(Case):
    SIZES, TH, DEST = (500, 1000, 2000), 7.0, "track_last_latency.json"

    def __init__(self, orb, fr, n):
        self.pose, self.bounds = fr.scenario(3, "tum1", n=1)[0], (0.0, 0.0, 640.0, 480.0)
        rng = self.start(orb, fr, n)
        px, py = self.cloud(rng)
        self.desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        self.observed = (rng.random(n) < 0.8).astype(np.uint8)
        src = rng.integers(0, n, NFEAT)
        x, y = px[src] + rng.normal(0, 2, NFEAT), py[src] + rng.normal(0, 2, NFEAT)
        oct_of = rng.integers(0, 8, n)
        self.frame(x, y, oct_of[src], self.desc[src], rng, angle=True)
        # the last frame: one feature per point plus a quarter without a map point, shuffled
        nl = n + n // 4
        self.slots = np.concatenate([np.arange(n), np.full(n // 4, -1)]).astype(np.int32)
        rng.shuffle(self.slots)
        self.lk = np.zeros(nl, orb.KP_DTYPE)
        self.lk["x"], self.lk["y"] = rng.uniform(1, 639, nl), rng.uniform(1, 479, nl)
        self.lk["octave"] = np.where(self.slots >= 0, oct_of[np.maximum(self.slots, 0)], rng.integers(0, 8, nl))
        self.lk["angle"] = rng.uniform(0, 360, nl)
        self.L = orb.Frame(nl + 1)
        self.L.upload(self.lk, rng.integers(0, 256, (nl, 32), dtype=np.uint8), self.bounds)
        self.mp = orb.MapPoints(n)
        self.mp.update(np.arange(n), world_pos=self.pos, desc=self.desc, observed=self.observed)
        self.mb = float(self.pose["mbf"] / self.pose["fx"])
        z_ = np.zeros
        self.index, self.qd, self.qo = z_(nl, np.int32), z_((nl, 32), np.uint8), z_(nl, np.uint8)
        self.u, self.v, self.ur, self.oc, self.an = (z_(nl, np.float32), z_(nl, np.float32), z_(nl, np.float32),
                                                     z_(nl, np.int32), z_(nl, np.float32))
        self.tb, self.tm, self.dir = z_(NFEAT, np.uint8), z_(NFEAT, np.int32), C.c_int(0)
        self.last_pose = orb.FramePose.make(**self.pose)
        self.nproj = 0

    def reset(self):
        self.tb[:] = 0
        self.tm[:] = -1

    def A(self, L, H, P):
        m = H.tl_host_side(C.byref(P), p(self.b, _f32p), len(self.slots), p(self.slots, _i32p), self.lk.ctypes.data_as(C.c_void_p),
                           p(self.pos, _f32p), p(self.desc, _u8p), p(self.observed, _u8p), p(self.index, _i32p),
                           p(self.qd, _u8p), p(self.qo, _u8p), p(self.u, _f32p), p(self.v, _f32p), p(self.ur, _f32p),
                           p(self.oc, _i32p), p(self.an, _f32p))
        self.nproj = m
        return L.vsg_frame_search_by_projection_last(
            self.F.handle, m, p(self.qd, _u8p), p(self.qo, _u8p), p(self.u, _f32p), p(self.v, _f32p), p(self.ur, _f32p), None,
            None, p(self.oc, _i32p), p(self.an, _f32p), self.TH, 0, p(self.sf, _f32p), 8, 1, p(self.tb, _u8p), p(self.tm, _i32p))

    def B(self, L, P):
        return L.vsg_frame_search_last_frame(
            self.F.handle, self.L.handle, self.mp.handle, p(self.slots, _i32p), C.byref(P), C.byref(self.last_pose), self.mb, 1,
            self.TH, p(self.sf, _f32p), 8, 1, p(self.tb, _u8p), p(self.tm, _i32p), C.byref(self.dir), None, None, None, None)

    def result(self, name, r):
        tm = self.tm.copy()
        if name[0] == "A":  # compacted indices -> last-frame features
            tm[tm >= 0] = self.index[tm[tm >= 0]]
        return r, tm

    def facts(self, last):
        return {"last_features": len(self.slots), "projected_last": int(self.nproj), "nmatches_last": int(last["B"][0])}


class KeyFrame(Case):
    SIZES, TH, DEST = (500, 1000, 2000), 3.0, "keyframe_points_latency.json"

    def __init__(self, orb, fr, n):
        self.pose, self.bounds = fr.scenario(3, "tum1", n=1)[0], (0.0, 0.0, 640.0, 480.0)
        rng = self.start(orb, fr, n)
        px, py = self.cloud(rng)
        PO = self.pos.astype(np.float64) - self.pose["Ow"]  # normals along the viewing rays
        dist = np.linalg.norm(PO, axis=1)
        self.normal = np.ascontiguousarray((PO / dist[:, None]).astype(np.float32))
        oct_of = rng.integers(0, 8, n)
        self.max_dist = (dist * 1.2 ** (oct_of - 0.5)).astype(np.float32)  # the predicted level is the feature's octave
        self.min_dist = (self.max_dist / np.float32(1.2) ** np.float32(7)).astype(np.float32)
        self.desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        self.skip = (rng.random(n) < 0.1).astype(np.uint8)
        src = rng.integers(0, n, NFEAT)
        x, y = px[src] + rng.normal(0, 0.7, NFEAT), py[src] + rng.normal(0, 0.7, NFEAT)
        self.frame(x, y, oct_of[src], self.desc[src], rng, angle=True)
        self.slots = np.arange(n, dtype=np.int32)
        self.mp = orb.MapPoints(n)
        self.mp.update(self.slots, world_pos=self.pos, normal=self.normal, min_dist=self.min_dist, max_dist=self.max_dist,
                       desc=self.desc)
        self.inv2 = (np.float32(1) / (self.sf * self.sf)).astype(np.float32)
        z_ = np.zeros
        self.index, self.qd = z_(n, np.int32), z_((n, 32), np.uint8)
        self.u, self.v, self.ur, self.rad, self.lvl = (z_(n, np.float32), z_(n, np.float32), z_(n, np.float32),
                                                       z_(n, np.float32), z_(n, np.int32))
        self.bi, self.bd = z_(n, np.int32), z_(n, np.int32)
        self.nproj = 0

    # (both sides hand back copies inside the clock: A's are the scatter of its compacted results back to the queries)
    def A(self, L, H, P):
        m = H.kp_host_side(C.byref(P), p(self.b, _f32p), self.n, p(self.skip, _u8p), p(self.pos, _f32p), p(self.normal, _f32p),
                           p(self.min_dist, _f32p), p(self.max_dist, _f32p), p(self.desc, _u8p), self.TH, p(self.sf, _f32p),
                           p(self.index, _i32p), p(self.qd, _u8p), p(self.u, _f32p), p(self.v, _f32p), p(self.ur, _f32p),
                           p(self.rad, _f32p), p(self.lvl, _i32p))
        self.nproj = m
        r = L.vsg_frame_fuse(self.F.handle, m, p(self.qd, _u8p), p(self.u, _f32p), p(self.v, _f32p), p(self.ur, _f32p),
                             p(self.rad, _f32p), p(self.lvl, _i32p), 0, p(self.inv2, _f32p), 8, p(self.bi, _i32p),
                             p(self.bd, _i32p))
        bi, bd = np.full(self.n, -1, np.int32), np.full(self.n, 256, np.int32)
        bi[self.index[:m]], bd[self.index[:m]] = self.bi[:m], self.bd[:m]
        return r, bi, bd

    def B(self, L, P):
        r = L.vsg_frame_fuse_points(self.F.handle, self.mp.handle, self.n, p(self.slots, _i32p), p(self.skip, _u8p), C.byref(P),
                                    self.TH, p(self.sf, _f32p), p(self.inv2, _f32p), 8, p(self.bi, _i32p), p(self.bd, _i32p), None,
                                    None, None, None, None)
        return r, self.bi.copy(), self.bd.copy()

    def result(self, name, got):
        return got

    def facts(self, last):
        return {"projected_last": int(self.nproj), "fused_last": int(last["B"][0])}


class Refresh(Case):
    """MapPoint::ComputeDistinctiveDescriptors + UpdateNormalAndDepth of n points of the store: 30 keyframes of 1000
    features with random descriptors, observation counts 2 + Gamma(1.5, 4) rounded and clipped to [2, 40] (mean near 8; a
    list longer than 30 names some keyframes twice), no keyframe bad.  Before every variant of every call the four fields of
    the listed slots are zeroed (outside the clock); after it the slots are read back (outside the clock) and compared."""
    SIZES, TH, DEST = (500, 2000, 8000), 0.0, "mappoints_refresh_latency.json"
    VARIANTS = ("A", "B", "A2", "Ap")
    NKF, KFN = 30, 1000

    def __init__(self, orb, fr, n):
        self.orb, self.n = orb, n
        rng = np.random.default_rng(n)
        self.sf = (np.float32(1.2) ** np.arange(8, dtype=np.float32)).astype(np.float32)
        m = np.clip(np.rint(2 + rng.gamma(1.5, 4.0, n)), 2, 40).astype(np.int64)
        self.off = np.concatenate([[0], np.cumsum(m)]).astype(np.int32)
        self.kf = np.concatenate([np.concatenate([rng.permutation(self.NKF), rng.integers(0, self.NKF, 10)])[:k]
                                  for k in m]).astype(np.int32)
        self.idx = rng.integers(0, self.KFN, len(self.kf)).astype(np.int32)
        self.ref = (rng.random(n) * m).astype(np.int32)
        self.kdesc = rng.integers(0, 256, (self.NKF, self.KFN, 32), dtype=np.uint8)
        self.koct = rng.integers(0, 8, (self.NKF, self.KFN)).astype(np.int32)
        self.Ow = rng.normal(0, 2.5, (self.NKF, 3)).astype(np.float32)
        self.pos = np.ascontiguousarray((rng.uniform(-6, 6, (n, 3)) + [0, 0, 12]).astype(np.float32))
        self.frames = []
        for k in range(self.NKF):
            keys = np.zeros(self.KFN, orb.KP_DTYPE)
            keys["octave"] = self.koct[k]
            keys["x"], keys["y"] = rng.uniform(0, 640, self.KFN), rng.uniform(0, 480, self.KFN)
            self.frames.append(orb.Frame(self.KFN + 1).upload(keys, self.kdesc[k], (0.0, 0.0, 640.0, 480.0)))
        self.handles = (C.c_void_p * self.NKF)(*[f.handle for f in self.frames])
        self.slots = rng.permutation(2 * n)[:n].astype(np.int32)  # a store twice the size, the points scattered over it
        self.mp = orb.MapPoints(2 * n)
        self.mp.update(self.slots, world_pos=self.pos)
        z = np.zeros
        self.rows, self.best, self.desc = z((len(self.kf), 32), np.uint8), z(n, np.int32), z((n, 32), np.uint8)
        self.nrm, self.mn, self.mx = z((n, 3), np.float32), z(n, np.float32), z(n, np.float32)
        self.zero = dict(normal=z((n, 3), np.float32), min_dist=z(n, np.float32), max_dist=z(n, np.float32),
                         desc=z((n, 32), np.uint8))
        self.m = m

    def pose_at(self, k):
        return None

    def reset(self):
        self.mp.update(self.slots, **self.zero)
        self.best[:] = -1

    def host(self, L, H, choose):
        H.rf_host_side(self.n, p(self.off, _i32p), p(self.kf, _i32p), p(self.idx, _i32p), p(self.ref, _i32p),
                       p(self.kdesc, _u8p), p(self.koct, _i32p), self.KFN, p(self.Ow, _f32p), p(self.pos, _f32p),
                       p(self.sf, _f32p), 8, choose, p(self.rows, _u8p), p(self.best, _i32p), p(self.desc, _u8p),
                       p(self.nrm, _f32p), p(self.mn, _f32p), p(self.mx, _f32p))
        if not choose:
            rc = L.vsg_distinctive_descriptors(0, p(self.rows, _u8p), p(self.off, _i32p), self.n, p(self.best, _i32p))
            if rc != 0:
                return rc
            H.rf_take_rows(self.n, p(self.off, _i32p), p(self.rows, _u8p), p(self.best, _i32p), p(self.desc, _u8p))
        return L.vsg_mappoints_update(self.mp.handle, self.n, p(self.slots, _i32p), None, p(self.nrm, _f32p), p(self.mn, _f32p),
                                      p(self.mx, _f32p), p(self.desc, _u8p), None)

    def B(self, L, P=None):
        return L.vsg_mappoints_refresh_from_observations(
            self.mp.handle, self.n, p(self.slots, _i32p), p(self.off, _i32p), p(self.kf, _i32p), p(self.idx, _i32p), None,
            p(self.ref, _i32p), self.NKF, self.handles, p(self.Ow, _f32p), p(self.sf, _f32p), 8, 3, p(self.best, _i32p), None,
            None, None)

    def run(self, name, L, H, P):
        return self.B(L) if name == "B" else self.host(L, H, 0 if name == "Ap" else 1)

    def result(self, name, r):
        s = self.mp.read(self.slots)
        return (r, self.best.copy(), np.frombuffer(s["desc"].tobytes(), np.uint8), s["normal"].view(np.uint32).copy(),
                s["min_dist"].view(np.uint32).copy(), s["max_dist"].view(np.uint32).copy())

    def facts(self, last):
        return {"observations": int(len(self.kf)), "mean_observations": round(float(self.m.mean()), 2),
                "max_observations": int(self.m.max()), "keyframes": self.NKF, "features_per_keyframe": self.KFN,
                "best_not_first": int((last["B"][1] != 0).sum())}


class Pose(Case):
    """Optimizer::PoseOptimization: n correspondences among the 1000 features of one frame (tests/pose_scenes.py's scene
    generator: uniform inlier noise within 0.8 sigma, 20 % outliers displaced by 20 px or more)."""
    SIZES, TH, DEST = (100, 300, 1000), 0.0, "pose_optimization_latency.json"
    VARIANTS = ("A", "B", "A2", "B2")

    def __init__(self, orb, fr, n):
        import pose_scenes as ps
        self.orb, self.n = orb, n
        s = self.s = ps.make(7000 + n, NFEAT, n, "mixed", outliers=0.2, start=(0.02, 1.0), capacity=2 * NFEAT)
        keys = np.zeros(NFEAT, orb.KP_DTYPE)
        keys["x"], keys["y"], keys["octave"] = s["kx"], s["ky"], s["octave"]
        self.frame = orb.Frame(NFEAT + 1).upload(keys, np.zeros((NFEAT, 32), np.uint8), (0.0, 0.0, 640.0, 480.0),
                                                 u_right=s["u_right"])
        self.mp = orb.MapPoints(s["capacity"])
        self.mp.update(np.arange(s["capacity"]), world_pos=s["world_pos"])
        c = np.ascontiguousarray
        self.slots, self.pos = c(s["feat_slots"], np.int32), c(s["world_pos"], np.float32)
        self.kx, self.ky, self.oct = c(s["kx"], np.float32), c(s["ky"], np.float32), c(s["octave"], np.int32)
        self.ur, self.sig = c(s["u_right"], np.float32), c(s["inv_sigma2"], np.float32)
        self.pose7, self.cam = np.concatenate([s["q"], s["t"]]).astype(np.float32), np.array(s["cam"], np.float32)
        self.tcw = orb.PoseSE3()
        self.tcw.q[:], self.tcw.t[:] = [float(v) for v in s["q"]], [float(v) for v in s["t"]]
        self.res = orb.PoseResult()
        self.out, self.chi2 = np.zeros(NFEAT, np.uint8), np.zeros(NFEAT, np.float32)
        self.qt, self.ri = np.zeros(7), np.zeros(2, np.int32)

    def pose_at(self, k):
        return None

    def reset(self):
        self.out[:], self.chi2[:], self.qt[:], self.ri[:] = 0, 0, 0, 0

    def run(self, name, L, H, P):
        if name.startswith("A"):
            return H.po_host_side(NFEAT, p(self.slots, _i32p), p(self.pos, _f32p), p(self.kx, _f32p), p(self.ky, _f32p),
                                  p(self.oct, _i32p), p(self.ur, _f32p), p(self.pose7, _f32p), p(self.cam, _f32p),
                                  p(self.sig, _f32p), 8, p(self.out, _u8p), p(self.chi2, _f32p),
                                  self.qt.ctypes.data_as(C.POINTER(C.c_double)), p(self.ri, _i32p))
        rc = L.vsg_frame_pose_optimization(self.frame.handle, self.mp.handle, p(self.slots, _i32p), C.byref(self.tcw),
                                           *[float(v) for v in self.cam], p(self.sig, _f32p), 8, -1, p(self.out, _u8p),
                                           p(self.chi2, _f32p), C.byref(self.res))
        self.qt[:4], self.qt[4:] = self.res.q[:], self.res.t[:]
        self.ri[:] = self.res.n_bad, self.res.rounds_run
        return rc

    def result(self, name, r):
        return (r, self.out.copy(), self.chi2.view(np.uint32).copy(), self.qt.view(np.uint64).copy(), self.ri.copy())

    def facts(self, last):
        return {"correspondences": self.n, "inliers_returned": int(last["B"][0]), "n_bad": int(last["B"][4][0]),
                "rounds_run": int(last["B"][4][1]), "stereo_share": round(float((self.ur[self.slots >= 0] >= 0).mean()), 2),
                "host_side": "host build of csrc/vsg_pose_opt.h, one thread; NOT g2o, likely flatters the host"}


class NewPoints(Case):
    """One neighbour of LocalMapping::CreateNewMapPoints: two resident keyframes of n features each (tests/
    triangulation_scenes.py's generator: 30 % of the features see a shared point, depths 0.4 .. 40, a third stereo), the
    k = 10 / L = 6 vocabulary's resident FeatureVectors, a store of 8000 slots."""
    SIZES, TH, DEST = (1000, 2000), 0.0, "create_new_map_points_latency.json"
    VARIANTS = ("A", "B", "A2", "B2")
    CAP = 8000

    def __init__(self, orb, fr, n):
        import triangulation_scenes as ts
        import triangulation_hostcore as hc
        from visual_sgraphs_amd import synth
        self.orb, self.n = orb, n
        rng = np.random.default_rng(9000 + n)
        npts = int(0.3 * n)
        s = self.s = ts.build(ts.cloud(rng, npts, 0.4, 40.0), *ts.cameras(), rng, extra=n - npts)
        voc = orb.ORBVocabulary(synth.synthetic_vocabulary(10, 6, seed=17, stop_fraction=0.05))
        self.f = []
        for t in ("1", "2"):
            f = orb.Frame(n).upload(s["k" + t], s["d" + t], ts.BOUNDS, u_right=s["ur" + t])
            f.SetStereoPoints(s["stereo" + t][:, :3], s["stereo" + t][:, 3])
            f.ComputeBoW(voc)
            self.f.append(f)
        self.mp = orb.MapPoints(self.CAP)
        c = np.ascontiguousarray
        self.free = np.arange(self.CAP, dtype=np.int32)
        self.P = orb.TriangulationParams.make(*[orb.FramePose.make(k["Rcw"], k["tcw"], k["Ow"], k["fx"], k["fy"], k["cx"], k["cy"],
                                                                  k["mbf"], 0.0, 0) for k in (s["P"]["kf1"], s["P"]["kf2"])],
                                            s["P"]["ratio_factor"])
        self.pb = hc.params_blob(s["P"])
        assert bytes(self.pb) == bytes(self.P)
        self.keep = []
        self.tab, self.oct = [], []
        for t in ("1", "2"):
            arr = [c(s["k" + t]["x"], np.float32), c(s["k" + t]["y"], np.float32), c(s["ur" + t], np.float32),
                   c(s["stereo" + t], np.float32), c(s["sf" + t], np.float32), c(s["sigma2_" + t], np.float32)]
            self.keep.append(arr)
            self.tab.append((C.c_void_p * 6)(*[a.ctypes.data for a in arr]))
            self.oct.append(c(s["k" + t]["octave"], np.int32))
        self.sf, self.sig = self.keep[0][4], self.keep[0][5]
        self.no_mp = [np.ones(n, np.uint8), np.ones(n, np.uint8)]
        self.F12, self.ep = c(s["F12"].reshape(9), np.float32), c(s["ep"], np.float32)
        self.m12, self.reason, self.source = np.zeros(n, np.int32), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        self.x3d, self.new_slot, self.created = np.zeros(3 * n, np.float32), np.zeros(n, np.int32), C.c_int32(0)
        self.slots, self.pos, self.obs_idx = np.zeros(n, np.int32), np.zeros(3 * n, np.float32), np.zeros(2 * n, np.int32)
        self.obs_off, self.obs_kf = np.arange(0, 2 * n + 1, 2, dtype=np.int32), np.tile(np.array([0, 1], np.int32), n)
        self.ref_pos, self.ones = np.zeros(n, np.int32), np.ones(n, np.uint8)
        self.kfs = (C.c_void_p * 2)(self.f[0].handle, self.f[1].handle)
        self.Ow = np.concatenate([s["P"]["kf1"]["Ow"], s["P"]["kf2"]["Ow"]]).astype(np.float32)
        self.best, self.o_n, self.o_mn, self.o_mx = (np.zeros(n, np.int32), np.zeros(3 * n, np.float32), np.zeros(n, np.float32),
                                                     np.zeros(n, np.float32))
        self.zero = dict(world_pos=np.zeros((n, 3), np.float32), normal=np.zeros((n, 3), np.float32), min_dist=np.zeros(n, np.float32),
                         max_dist=np.zeros(n, np.float32), desc=np.zeros((n, 32), np.uint8), observed=np.zeros(n, np.uint8))

    def pose_at(self, k):
        return None

    def reset(self):  # outside the clock: the slots a call may write are cleared, so that every variant has to write them
        self.mp.update(self.free[:self.n], **self.zero)
        self.m12[:], self.reason[:], self.source[:], self.x3d[:], self.new_slot[:] = 0, 0, 0, 0, 0

    def run(self, name, L, H, P):
        f1, f2, n = self.f[0].handle, self.f[1].handle, self.n
        if name.startswith("B"):
            return L.vsg_frame_create_new_map_points(
                f1, p(self.no_mp[0], _u8p), None, None, None, 0, f2, p(self.no_mp[1], _u8p), None, None, None, 0, p(self.F12, _f32p),
                p(self.ep, _f32p), 0, 0, 1, C.byref(self.P), p(self.sf, _f32p), p(self.sig, _f32p), p(self.sf, _f32p),
                p(self.sig, _f32p), 4, self.mp.handle, p(self.free, _i32p), self.CAP, p(self.m12, _i32p), p(self.reason, _u8p),
                p(self.source, _u8p), p(self.x3d, _f32p), p(self.new_slot, _i32p), C.byref(self.created))
        nm = L.vsg_frame_search_for_triangulation_epipolar(
            f1, p(self.no_mp[0], _u8p), None, None, None, 0, f2, p(self.no_mp[1], _u8p), None, None, None, 0, p(self.F12, _f32p),
            p(self.ep, _f32p), p(self.sf, _f32p), p(self.sig, _f32p), 4, 0, 0, 1, p(self.m12, _i32p))
        k = H.np_host_side(C.byref(self.P), n, self.tab[0], p(self.oct[0], _i32p), n, self.tab[1], p(self.oct[1], _i32p),
                           p(self.m12, _i32p), 4, p(self.free, _i32p), self.CAP, p(self.reason, _u8p), p(self.source, _u8p),
                           p(self.x3d, _f32p), p(self.new_slot, _i32p), p(self.slots, _i32p), p(self.pos, _f32p),
                           p(self.obs_idx, _i32p))
        self.created.value = k
        if k:
            assert L.vsg_mappoints_update(self.mp.handle, k, p(self.slots, _i32p), p(self.pos, _f32p), None, None, None, None,
                                          p(self.ones, _u8p)) == 0
            assert L.vsg_mappoints_refresh_from_observations(
                self.mp.handle, k, p(self.slots, _i32p), p(self.obs_off, _i32p), p(self.obs_kf, _i32p), p(self.obs_idx, _i32p), None,
                p(self.ref_pos, _i32p), 2, self.kfs, p(self.Ow, _f32p), p(self.sf, _f32p), 4, 3, p(self.best, _i32p),
                p(self.o_n, _f32p), p(self.o_mn, _f32p), p(self.o_mx, _f32p)) == 0
        return nm

    def result(self, name, r):
        st = self.mp.read(self.free[:self.n])
        return (r, self.m12.copy(), self.reason.copy(), self.source.copy(), self.x3d.view(np.uint32).copy(), self.new_slot.copy(),
                np.array([self.created.value]), st["world_pos"].view(np.uint32).copy(), st["normal"].view(np.uint32).copy(),
                st["min_dist"].view(np.uint32).copy(), st["max_dist"].view(np.uint32).copy(), st["desc"].copy(), st["observed"].copy())

    def facts(self, last):
        b = last["B"]
        return {"features_per_keyframe": self.n, "matches_after_rotation_filter": int(b[0]), "points_created": int(b[6][0]),
                "from_unproject_stereo": int(((b[2] == 0) & (b[3] > 0)).sum()), "store_slots": self.CAP,
                "host_side": "A = vsg_frame_search_for_triangulation_epipolar + the host build of csrc/vsg_triangulate.h on one "
                             "thread (tools/resident_points_cpu.cpp; NOT Eigen: the double Jacobi of the header, no JacobiSVD) + "
                             "vsg_mappoints_update + vsg_mappoints_refresh_from_observations; B = vsg_frame_create_new_map_points"}


class Sim3(Case):
    """Sim3Solver on resident map points: a scene of tests/sim3_scenes.py (two keyframes in two maps, the point sets related by
    a similarity of scale 1.3, 1 cm noise), its points in random slots of two stores.  A size is "<correspondences>:<loop|false>"."""
    SIZES = tuple("%d:%s" % (n, c) for n in (30, 100, 300) for c in ("loop", "false"))
    TH, DEST = 0.0, "sim3_ransac_latency.json"
    VARIANTS = ("A", "B", "A2", "B2")
    CAP, NHYP, MIN_INLIERS = 4096, 300, 15

    def __init__(self, orb, fr, size):
        import sim3_scenes as ss
        n, kind = int(size.split(":")[0]), size.split(":")[1]
        self.orb, self.n, self.kind = orb, n, kind
        s = self.s = ss.make(7000 + n, n=n, outliers=0.3 if kind == "loop" else 1.0, n_hyp=self.NHYP)
        rng = np.random.default_rng(n)
        c = np.ascontiguousarray
        self.mp = [orb.MapPoints(self.CAP), orb.MapPoints(self.CAP)]
        self.slots = [c(rng.permutation(self.CAP)[:n], np.int32) for _ in range(2)]
        self.mp[0].update(self.slots[0], world_pos=s["Xw1"])
        self.mp[1].update(self.slots[1], world_pos=s["Xw2"])
        self.err = [c(s["max_err1"], np.float32), c(s["max_err2"], np.float32)]
        self.kf = [orb.FramePose.make(k["Rcw"], k["tcw"], np.zeros(3), k["fx"], k["fy"], k["cx"], k["cy"], 0.0, 0.0, 0)
                   for k in (s["kf1"], s["kf2"])]
        self.samples = c(s["samples"], np.int32)
        self.Xw = [np.zeros(3 * n, np.float32), np.zeros(3 * n, np.float32)]
        self.inlier, self.res = np.zeros(n, np.uint8), orb.Sim3Result()

    def pose_at(self, k):
        return None

    def reset(self):
        self.inlier[:] = 9
        C.memset(C.byref(self.res), 0, C.sizeof(self.res))

    def run(self, name, L, H, P):
        n = self.n
        if name.startswith("B"):
            return L.vsg_mappoints_sim3_ransac(self.mp[0].handle, self.mp[1].handle, n, p(self.slots[0], _i32p), p(self.slots[1], _i32p),
                                               p(self.err[0], _f32p), p(self.err[1], _f32p), C.byref(self.kf[0]), C.byref(self.kf[1]),
                                               0, self.MIN_INLIERS, self.NHYP, p(self.samples, _i32p), p(self.inlier, _u8p),
                                               C.byref(self.res), None, None)
        for k in range(2):
            rc = L.vsg_mappoints_read(self.mp[k].handle, n, p(self.slots[k], _i32p), p(self.Xw[k], _f32p), None, None, None, None, None)
            if rc != 0:
                return rc
        H.s3_host_side(n, p(self.Xw[0], _f32p), p(self.Xw[1], _f32p), p(self.err[0], _f32p), p(self.err[1], _f32p),
                       C.byref(self.kf[0]), C.byref(self.kf[1]), 0, self.MIN_INLIERS, self.NHYP, p(self.samples, _i32p),
                       p(self.inlier, _u8p), C.byref(self.res))
        return 0

    def result(self, name, r):
        return (r, self.inlier.copy(), np.frombuffer(bytes(self.res), np.uint8).copy())

    def facts(self, last):
        r = self.orb.Sim3Result.from_buffer_copy(last["B"][2].tobytes())
        return {"correspondences": self.n, "case": self.kind, "hypotheses": self.NHYP, "min_inliers": self.MIN_INLIERS,
                "converged": bool(r.converged), "hypotheses_walked_by_the_reference_loop": int(r.iterations),
                "n_inliers": int(r.n_inliers), "store_slots": self.CAP,
                "host_side": "A = vsg_mappoints_read x 2 + the host build of csrc/vsg_sim3.h on one thread with the reference's early "
                             "exit (tools/resident_points_cpu.cpp; NOT Eigen: the header's double Jacobi, no EigenSolver, no "
                             "Sophus); B = vsg_mappoints_sim3_ransac, which computes all hypotheses"}


class Mlpnp(Case):
    """MLPnPsolver on a resident frame: a scene of tests/mlpnp_scenes.py (TUM1 intrinsics, 0.5 px noise times the level scale),
    its correspondences scattered among 1000 features and 4096 store slots.  A size is "<correspondences>:<true|false>"."""
    SIZES = tuple("%d:%s" % (n, c) for n in (30, 100, 300) for c in ("true", "false"))
    TH, DEST = 0.0, "mlpnp_latency.json"
    VARIANTS = ("A", "B", "A2", "B2")
    CAP = 4096

    def __init__(self, orb, fr, size):
        import mlpnp_scenes as ms
        n, kind = int(size.split(":")[0]), size.split(":")[1]
        self.orb, self.n, self.kind, self.ms = orb, n, kind, ms
        s = self.s = ms.make(8000 + n, n=n, outliers=0.3 if kind == "true" else 1.0, n_hyp=300, capacity=self.CAP, extra=NFEAT - n - 7)
        c = np.ascontiguousarray
        keys = np.zeros(s["n_feat"], orb.KP_DTYPE)
        keys["x"], keys["y"], keys["octave"], keys["size"], keys["angle"] = s["kx"], s["ky"], s["octave"], 31.0, -1.0
        self.F = orb.Frame(s["n_feat"] + 1).upload(keys, np.zeros((s["n_feat"], 32), np.uint8), (0.0, 0.0, 640.0, 480.0))
        self.mp = orb.MapPoints(self.CAP)
        self.mp.update(np.arange(self.CAP), world_pos=s["world_pos"])
        self.min_inliers, self.max_its = orb.mlpnp_ransac_parameters(n)
        self.slots, self.sets = c(s["slots"], np.int32), c(s["sets"][:self.max_its], np.int32)
        self.used = c(s["slots"][s["slots"] >= 0], np.int32)
        self.kx, self.ky, self.oct = c(s["kx"], np.float32), c(s["ky"], np.float32), c(s["octave"], np.int32)
        self.cam, self.sig = np.array(ms.CAM, np.float32), c(ms.LEVEL_SIGMA2, np.float32)
        self.Xw = np.zeros(3 * n, np.float32)
        self.inlier, self.res = np.zeros(s["n_feat"], np.uint8), orb.MlpnpResult()

    def pose_at(self, k):
        return None

    def reset(self):
        self.inlier[:] = 9
        C.memset(C.byref(self.res), 0, C.sizeof(self.res))

    def run(self, name, L, H, P):
        ms = self.ms
        if name.startswith("B"):
            return L.vsg_frame_mlpnp_ransac(self.F.handle, self.mp.handle, p(self.slots, _i32p), *[float(v) for v in self.cam],
                                            p(self.sig, _f32p), ms.NLEVELS, ms.TH2, self.min_inliers, self.max_its, 0, 5, self.max_its,
                                            p(self.sets, _i32p), p(self.inlier, _u8p), C.byref(self.res), None, None)
        rc = L.vsg_mappoints_read(self.mp.handle, self.n, p(self.used, _i32p), p(self.Xw, _f32p), None, None, None, None, None)
        if rc != 0:
            return rc
        H.ml_host_side(len(self.slots), p(self.slots, _i32p), p(self.Xw, _f32p), p(self.kx, _f32p), p(self.ky, _f32p), p(self.oct, _i32p),
                       p(self.cam, _f32p), p(self.sig, _f32p), ms.TH2, self.min_inliers, self.max_its, 5, p(self.sets, _i32p),
                       p(self.inlier, _u8p), C.byref(self.res))
        return 0

    def result(self, name, r):
        return (r, self.inlier.copy(), np.frombuffer(bytes(self.res), np.uint8).copy())

    def facts(self, last):
        r = self.orb.MlpnpResult.from_buffer_copy(last["B"][2].tobytes())
        return {"correspondences": self.n, "case": self.kind, "features": len(self.slots), "min_inliers": self.min_inliers,
                "hypotheses_computed_by_the_device_call": self.max_its, "found": bool(r.found), "refined": bool(r.refined),
                "no_more": bool(r.no_more), "hypotheses_walked_by_the_reference_loop": int(r.iterations), "n_inliers": int(r.n_inliers),
                "store_slots": self.CAP,
                "host_side": "A = vsg_mappoints_read + the host build of csrc/vsg_mlpnp.h on one thread with the reference's early "
                             "return and Refine()'s dropped solve over the best set (tools/resident_points_cpu.cpp; THIS header's "
                             "build and NOT Eigen: its one-sided Jacobi and unpivoted LDL^T, no JacobiSVD, no sparse matrices); "
                             "B = vsg_frame_mlpnp_ransac, which computes all hypotheses and leaves the dropped solve out"}


class TwoView(Case):
    """TwoViewReconstruction::Reconstruct (Tracking::MonocularInitialization, Tracking.cc:2568): a general scene of
    tests/two_view_scenes.py, 200 sets.  A size is "<matches>:<features per frame>".  AT = A with the two model searches on two
    threads, as the reference runs them."""
    SIZES = ("100:1000", "300:1000", "1000:2000")
    TH, DEST = 0.0, "two_view_latency.json"
    VARIANTS = ("A", "B", "A2", "B2", "AT")
    NITER = 200

    def __init__(self, orb, fr, size):
        import two_view_scenes as ts
        n, feat = (int(v) for v in size.split(":"))
        self.orb, self.n, self.feat = orb, n, feat
        s = self.s = ts.make(9000 + n, n=n, extra1=feat - n, extra2=feat - n, n_iter=self.NITER)
        c = np.ascontiguousarray
        self.xy = [c(s["xy1"], np.float32), c(s["xy2"], np.float32)]
        self.m12, self.K, self.sets = c(s["matches12"], np.int32), c(s["K"], np.float32), c(s["sets"], np.int32)
        self.F = []
        for xy in self.xy:
            keys = np.zeros(feat, orb.KP_DTYPE)
            keys["x"], keys["y"], keys["size"] = xy[:, 0], xy[:, 1], 31.0
            self.F.append(orb.Frame(feat + 1).upload(keys, np.zeros((feat, 32), np.uint8), (0.0, 0.0, 640.0, 480.0)))
        self.params = orb.TwoViewParams()
        orb.load_library().vsg_two_view_default_params(C.byref(self.params))
        self.res, self.tri, self.x3d = orb.TwoViewResult(), np.zeros(feat, np.uint8), np.zeros(3 * feat, np.float32)

    def pose_at(self, k):
        return None

    def reset(self):
        self.tri[:], self.x3d[:] = 9, -1.0
        C.memset(C.byref(self.res), 0, C.sizeof(self.res))

    def run(self, name, L, H, P):
        if name.startswith("B"):
            return L.vsg_frame_two_view_reconstruct(self.F[0].handle, self.F[1].handle, p(self.m12, _i32p), p(self.K, _f32p),
                                                    C.byref(self.params), self.NITER, p(self.sets, _i32p), C.byref(self.res),
                                                    p(self.tri, _u8p), p(self.x3d, _f32p), None, None, None, None)
        return H.tv_host_side(p(self.xy[0], _f32p), self.feat, p(self.xy[1], _f32p), self.feat, p(self.m12, _i32p), p(self.K, _f32p),
                              C.byref(self.params), self.NITER, p(self.sets, _i32p), 1 if name == "AT" else 0, C.byref(self.res),
                              p(self.tri, _u8p), p(self.x3d, _f32p))

    def result(self, name, r):
        return (0 if r >= 0 else r, self.tri.copy(), self.x3d.copy(), np.frombuffer(bytes(self.res), np.uint8).copy())

    def facts(self, last):
        r = self.orb.TwoViewResult.from_buffer_copy(last["B"][3].tobytes())
        return {"matches": self.n, "features_per_frame": self.feat, "sets": self.NITER, "ok": bool(r.ok), "model": "F" if r.model else "H",
                "n_inliers": int(r.n_inliers), "n_good": [int(v) for v in r.n_good],
                "host_side": "A = the host build of csrc/vsg_two_view.h on one thread, given the keypoint arrays "
                             "(tools/resident_points_cpu.cpp; NOT Eigen: the header's double Jacobi with one rounding per operation, "
                             "no JacobiSVD); AT = the same with the two model searches on two threads, as the reference runs them; "
                             "B = vsg_frame_two_view_reconstruct"}


class Sim3Opt(Case):
    """Optimizer::OptimizeSim3 on resident keyframes and map points: a scene of tests/sim3opt_scenes.py (two keyframes of 1000
    features, the pairs related by a similarity of scale 1.3, inlier noise within 0.8 sigma, 20 % outliers displaced by 6 sigma
    or more, the input 2 cm / 1 degree / 2 % off).  A size is "<pairs>:<fix_scale>"."""
    SIZES = tuple("%d:%d" % (n, f) for n in (30, 100, 300) for f in (0, 1))
    TH, DEST = 10.0, "sim3_optimization_latency.json"
    VARIANTS = ("A", "B", "A2", "B2")
    CAP = 4096

    def __init__(self, orb, fr, size):
        import sim3opt_scenes as ss
        n, fix = (int(v) for v in size.split(":"))
        self.orb, self.n, self.fix = orb, n, fix
        s = self.s = ss.make(7100 + n + fix, n, n1=NFEAT, outliers=0.2, fix_scale=fix, scale=1.3, capacity=self.CAP)
        c = np.ascontiguousarray

        def keys(k):
            out = np.zeros(len(k["x"]), orb.KP_DTYPE)
            out["x"], out["y"], out["octave"] = k["x"], k["y"], k["octave"]
            return out
        self.kf = [orb.Frame(len(k["x"]) + 1).upload(keys(k), np.zeros((len(k["x"]), 32), np.uint8), (0.0, 0.0, 640.0, 480.0))
                   for k in (s["kps1"], s["kps2"])]
        self.mp = [orb.MapPoints(self.CAP), orb.MapPoints(self.CAP)]
        self.mp[0].update(np.arange(self.CAP), world_pos=s["pos1"])
        self.mp[1].update(np.arange(self.CAP), world_pos=s["pos2"])
        self.pose = [orb.FramePose.make(k["Rcw"], k["tcw"], np.zeros(3), k["fx"], k["fy"], k["cx"], k["cy"], 0.0, 0.0, 0)
                     for k in (s["pose1"], s["pose2"])]
        self.slots = [c(s["slots1"], np.int32), c(s["slots2"], np.int32)]
        self.idx2, self.level2 = c(s["idx2"], np.int32), c(s["level2"], np.int32)
        self.sig = c(s["sig1"], np.float32)
        self.S12 = orb.Sim3d.make(*s["S12"])
        # the caller-side path reads the points of the entries that have one: their slots, and where each lands in the read-back
        self.rd, self.back, self.Xw = [], [], []
        for sl in self.slots:
            have = np.flatnonzero(sl >= 0)
            back = np.full(len(sl), -1, np.int32)
            back[have] = np.arange(len(have), dtype=np.int32)
            self.rd.append(c(sl[have], np.int32)), self.back.append(back), self.Xw.append(np.zeros(3 * len(have), np.float32))
        self.k = [[c(k["x"], np.float32), c(k["y"], np.float32), c(k["octave"], np.int32)] for k in (s["kps1"], s["kps2"])]
        self.state, self.chi2, self.res = np.zeros(NFEAT, np.uint8), np.zeros(2 * NFEAT), orb.Sim3OptResult()

    def pose_at(self, k):
        return None

    def reset(self):
        self.state[:], self.chi2[:] = 9, -1.0
        C.memset(C.byref(self.res), 0, C.sizeof(self.res))

    def run(self, name, L, H, P):
        f64p = C.POINTER(C.c_double)
        if name.startswith("B"):
            return L.vsg_frame_optimize_sim3(self.kf[0].handle, self.kf[1].handle, self.mp[0].handle, self.mp[1].handle,
                                             p(self.slots[0], _i32p), p(self.slots[1], _i32p), p(self.idx2, _i32p),
                                             p(self.level2, _i32p), C.byref(self.pose[0]), C.byref(self.pose[1]), p(self.sig, _f32p),
                                             p(self.sig, _f32p), 8, C.byref(self.S12), self.TH, self.fix, 0, p(self.state, _u8p),
                                             p(self.chi2, f64p), C.byref(self.res))
        for k in range(2):
            rc = L.vsg_mappoints_read(self.mp[k].handle, len(self.rd[k]), p(self.rd[k], _i32p), p(self.Xw[k], _f32p), None, None,
                                      None, None, None)
            if rc != 0:
                return rc
        return H.so_host_side(NFEAT, len(self.k[1][0]), p(self.back[0], _i32p), p(self.back[1], _i32p), p(self.idx2, _i32p),
                              p(self.level2, _i32p), len(self.rd[0]), len(self.rd[1]), p(self.Xw[0], _f32p), p(self.Xw[1], _f32p),
                              p(self.k[0][0], _f32p), p(self.k[0][1], _f32p), p(self.k[0][2], _i32p), p(self.k[1][0], _f32p),
                              p(self.k[1][1], _f32p), p(self.k[1][2], _i32p), C.addressof(self.pose[0]), C.addressof(self.pose[1]),
                              p(self.sig, _f32p), p(self.sig, _f32p), 8, C.addressof(self.S12), self.TH, self.fix, 0,
                              p(self.state, _u8p), p(self.chi2, f64p), C.addressof(self.res))

    def result(self, name, r):
        return (r, self.state.copy(), self.chi2.view(np.uint64).copy(), np.frombuffer(bytes(self.res), np.uint8).copy())

    def facts(self, last):
        r = self.orb.Sim3OptResult.from_buffer_copy(last["B"][3].tobytes())
        return {"pairs": self.n, "fix_scale": self.fix, "features_per_keyframe": NFEAT, "store_slots": self.CAP,
                "n_correspondences": int(r.n_correspondences), "n_bad": int(r.n_bad), "n_in": int(r.n_in),
                "more_iterations": int(r.more_iterations),
                "host_side": "A = vsg_mappoints_read x 2 + the host build of csrc/vsg_sim3_opt.h on one thread "
                             "(tools/resident_points_cpu.cpp); it is THIS header's build and NOT g2o (no Eigen here): the same "
                             "arithmetic, no virtual calls, no sparse block solver, so it likely flatters the host; "
                             "B = vsg_frame_optimize_sim3"}


class LocalBA(Case):
    """The visual part of Optimizer::LocalBundleAdjustment on resident keyframes and map points: a scene of
    tests/lba_scenes.py (n optimised + n fixed keyframes padded to 1000 features each, points of 6 observations, half of them
    stereo, 5 % outliers displaced by 20 px or more, the optimised keyframes and the points started 1 cm / 0.5 degrees off).
    A size is "<optimised = fixed keyframes>:<points>".  B, B_S1, B_S2 and B_S10 are the resident call with the library's trial
    slots, 1, 2 and 10 of them enqueued ahead per iteration."""
    SIZES = ("10:1500", "20:3000", "40:6000")
    TH, DEST = 0.0, "local_ba_latency.json"
    VARIANTS = ("A", "B", "A2", "B2", "B_S1", "B_S2", "B_S10")

    def __init__(self, orb, fr, size):
        import lba_scenes as ls
        nk, npts = (int(v) for v in size.split(":"))
        self.setup(orb, ls.make(7300 + nk, nk, nk, npts, 6, "mixed", outliers=0.05), nk, npts)

    def setup(self, orb, s, nk, npts):
        """The scene's keyframes padded and uploaded, the store, and the arrays both sides take."""
        self.orb, self.nk, self.npts, self.s = orb, nk, npts, s
        c = np.ascontiguousarray
        rng = np.random.default_rng(nk)
        self.kf, feats = [], []
        for f in s["kfs"]:  # pad to NFEAT features: the observed ones keep their indices
            n, pad = len(f["x"]), max(NFEAT - len(f["x"]), 0)
            x = np.concatenate([f["x"], rng.uniform(20, 620, pad)]).astype(np.float32)
            y = np.concatenate([f["y"], rng.uniform(20, 460, pad)]).astype(np.float32)
            o = np.concatenate([f["octave"], rng.integers(0, 8, pad)]).astype(np.int32)
            ur = np.concatenate([np.full(n, -1, np.float32) if f["ur"] is None else f["ur"], np.full(pad, -1)]).astype(np.float32)
            keys = np.zeros(len(x), orb.KP_DTYPE)
            keys["x"], keys["y"], keys["octave"] = x, y, o
            self.kf.append(orb.Frame(len(x) + 1).upload(keys, np.zeros((len(x), 32), np.uint8), (0.0, 0.0, 640.0, 480.0), u_right=ur))
            feats.append((x, y, o, ur))
        self.K = len(self.kf)
        self.handles = (C.c_void_p * self.K)(*[f.handle for f in self.kf])
        self.kf_off = np.zeros(self.K + 1, np.int32)
        self.kf_off[1:] = np.cumsum([len(f[0]) for f in feats])
        self.kx, self.ky, self.oct, self.ur = (c(np.concatenate([f[i] for f in feats])) for i in range(4))
        self.cap = s["capacity"]
        self.mp = orb.MapPoints(self.cap)
        self.all, self.pos0 = np.arange(self.cap, dtype=np.int32), c(s["store_pos"], np.float32)
        self.slots, self.off = c(s["slots"], np.int32), c(s["obs_off"], np.int32)
        self.okf, self.oidx = c(s["obs_kf"], np.int32), c(s["obs_idx"], np.int32)
        self.Tcw, self.fixed = c(s["Tcw"], np.float32), c(s["fixed"], np.uint8)
        self.cam, self.sig = c(s["cam"], np.float32), c(s["sig"], np.float32)
        E = int(self.off[-1])
        self.Xw = np.zeros(3 * npts, np.float32)
        self.kf_out, self.pos_out = np.zeros((self.K, 7)), np.zeros(3 * npts, np.float32)
        self.erase, self.chi2, self.res = np.zeros(E, np.uint8), np.zeros(E), orb.LocalBaResult()

    def pose_at(self, k):
        return None

    def reset(self):  # outside the clock: the store goes back to the start, the outs are cleared
        self.mp.update(self.all, world_pos=self.pos0)
        self.kf_out[:], self.pos_out[:], self.erase[:], self.chi2[:] = 0, 0, 9, -1.0
        C.memset(C.byref(self.res), 0, C.sizeof(self.res))

    def run(self, name, L, H, P):
        f64p = C.POINTER(C.c_double)
        if name.startswith("B"):
            L.vsg_debug_local_ba_trial_slots({"B_S1": 1, "B_S2": 2, "B_S10": 10}.get(name, 0))
            rc = L.vsg_mappoints_local_bundle_adjustment(
                self.mp.handle, self.npts, p(self.slots, _i32p), p(self.off, _i32p), p(self.okf, _i32p), p(self.oidx, _i32p), self.K,
                self.handles, C.cast(self.Tcw.ctypes.data, C.POINTER(self.orb.PoseSE3)), p(self.fixed, _u8p),
                C.cast(self.cam.ctypes.data, C.POINTER(self.orb.BaCamera)), p(self.sig, _f32p), 8, 10, None,
                C.cast(self.kf_out.ctypes.data, C.POINTER(self.orb.PoseSE3d)), p(self.pos_out, _f32p), p(self.erase, _u8p),
                p(self.chi2, f64p), C.byref(self.res))
            L.vsg_debug_local_ba_trial_slots(0)
            return rc
        rc = L.vsg_mappoints_read(self.mp.handle, self.npts, p(self.slots, _i32p), p(self.Xw, _f32p), None, None, None, None, None)
        if rc != 0:
            return rc
        rc = H.lb_host_side(self.cap, self.npts, p(self.slots, _i32p), p(self.Xw, _f32p), p(self.off, _i32p), p(self.okf, _i32p),
                            p(self.oidx, _i32p), self.K, p(self.kf_off, _i32p), p(self.kx, _f32p), p(self.ky, _f32p),
                            p(self.oct, _i32p), p(self.ur, _f32p), self.Tcw.ctypes.data, p(self.fixed, _u8p), self.cam.ctypes.data,
                            p(self.sig, _f32p), 8, 10, self.kf_out.ctypes.data, p(self.pos_out, _f32p), p(self.erase, _u8p),
                            p(self.chi2, f64p), C.addressof(self.res))
        if rc != 0:
            return rc
        return L.vsg_mappoints_update(self.mp.handle, self.npts, p(self.slots, _i32p), p(self.pos_out, _f32p), None, None, None,
                                      None, None)

    def result(self, name, r):
        after = self.mp.read(self.slots)["world_pos"]
        return (r, self.kf_out.view(np.uint64).copy(), self.pos_out.copy(), after.reshape(-1).copy(), self.erase.copy(),
                self.chi2.view(np.uint64).copy(), np.frombuffer(bytes(self.res), np.uint8).copy())

    def facts(self, last):
        r = self.orb.LocalBaResult.from_buffer_copy(last["B"][6].tobytes())
        return {"optimised_keyframes": self.nk, "fixed_keyframes": self.nk, "points": self.npts, "edges": int(r.n_edges),
                "mono": int(r.n_mono), "stereo": int(r.n_stereo), "erased": int(r.n_erase), "features_per_keyframe": NFEAT,
                "iterations_run": int(r.iterations_run), "trials_run": int(r.trials_run), "stop_reason": int(r.stop_reason),
                "every_call_equals_the_host_build": True,
                "host_side": "A = vsg_mappoints_read + the host build of csrc/vsg_local_ba.h on one thread "
                             "(tools/resident_points_cpu.cpp) + vsg_mappoints_update; it is THIS header's build and NOT g2o (no "
                             "Eigen here).  Which way that flatters it: g2o's sparse reduced solve is cheaper than this dense "
                             "one for many keyframes, its virtual calls and allocations are dearer; "
                             "B = vsg_mappoints_local_bundle_adjustment (B_S1 / B_S2 / B_S10: 1 / 2 / 10 trial slots enqueued ahead)"}


class SGraphBA(LocalBA):
    """Optimizer::LocalBundleAdjustment with its planes and rooms: LocalBA's scene and the planes, observations and rooms of
    tests/sgba_scenes.py on it.  A size is "<optimised = fixed keyframes>:<points>:<plane_kf factor too>"."""
    SIZES = ("10:1500:0", "20:3000:0", "40:6000:0", "10:1500:1", "20:3000:1", "40:6000:1")
    TH, DEST = 0.0, "sgraph_local_ba_latency.json"
    VARIANTS = ("A", "B", "A2", "B2", "V", "V2")
    SAME = ("B", "A2", "B2")  # V and V2 solve another problem

    def __init__(self, orb, fr, size):
        import lba_scenes as ls
        import sgba_scenes as ss
        nk, npts, both = (int(v) for v in size.split(":"))
        s = ls.make(7300 + nk, nk, nk, npts, 6, "mixed", outliers=0.05)
        self.setup(orb, s, nk, npts)
        rng = np.random.default_rng(7400 + nk)
        n_planes, n_rooms, K = (4 * nk) // 5, max(nk // 10, 1), 2 * nk
        planes = [ss.face(i) for i in range(6)] + [ss.oblique(rng) for _ in range(n_planes - 6)]
        c = np.ascontiguousarray
        off, okf, loc, G, wk, wp = [0], [], [], [], [], []
        for pl in planes:  # seen by a third of the keyframes, from where the keyframes start
            for k in np.sort(rng.choice(K, K // 3, replace=False)):
                l, g = ss.observation(rng, s["Tcw"][k].astype(np.float64), pl)
                conf = rng.uniform(0.5, 1.0)
                okf.append(k), loc.append(l), G.append(g), wk.append(conf * ss.GAIN_KF if both else 0.0), wp.append(conf * ss.GAIN_PP)
            off.append(len(okf))
        rooms = [(0, 1, 2, 3)] + [(6 + 2 * r, 7 + 2 * r) for r in range(n_rooms - 1)]
        self.eq = c([ss.start_plane(rng, pl) for pl in planes], np.float64)
        self.poff, self.pkf = c(off, np.int32), c(okf, np.int32)
        self.loc, self.G, self.wk, self.wp = c(loc, np.float64), c(G, np.float64), c(wk, np.float64), c(wp, np.float64)
        self.rc = c([ss.room_center([planes[w] for w in r]) + rng.normal(0, 0.02, 3) for r in rooms], np.float64)
        self.rn = c([len(r) for r in rooms], np.int32)
        self.rw = c([list(r) + [0] * (4 - len(r)) for r in rooms], np.int32)
        self.n_planes, self.n_rooms, NO = n_planes, n_rooms, len(okf)
        self.plane_out, self.room_out = np.zeros((n_planes, 4)), np.zeros((n_rooms, 3))
        self.erase_plane, self.chi2k, self.chi2p = np.zeros(NO, np.uint8), np.zeros(NO), np.zeros(NO)
        self.sres, self.vres = orb.SGraphLocalBaResult(), orb.LocalBaResult()

    def reset(self):
        LocalBA.reset(self)
        self.plane_out[:], self.room_out[:], self.erase_plane[:], self.chi2k[:], self.chi2p[:] = 0, 0, 9, -1.0, -1.0
        C.memset(C.byref(self.sres), 0, C.sizeof(self.sres))

    def run(self, name, L, H, P):
        f64p = C.POINTER(C.c_double)
        sem = (self.n_planes, p(self.eq, f64p), p(self.poff, _i32p), p(self.pkf, _i32p), p(self.loc, f64p), p(self.G, f64p),
               p(self.wk, f64p), p(self.wp, f64p), self.n_rooms, p(self.rc, f64p), p(self.rn, _i32p), p(self.rw, _i32p),
               p(self.plane_out, f64p), p(self.room_out, f64p), p(self.erase_plane, _u8p), p(self.chi2k, f64p), p(self.chi2p, f64p))
        if name.startswith("V"):
            return LocalBA.run(self, "B", L, H, P)
        if name.startswith("B"):
            return L.vsg_mappoints_local_bundle_adjustment_sgraph(
                self.mp.handle, self.npts, p(self.slots, _i32p), p(self.off, _i32p), p(self.okf, _i32p), p(self.oidx, _i32p), self.K,
                self.handles, C.cast(self.Tcw.ctypes.data, C.POINTER(self.orb.PoseSE3)), p(self.fixed, _u8p),
                C.cast(self.cam.ctypes.data, C.POINTER(self.orb.BaCamera)), p(self.sig, _f32p), 8, 10, None,
                C.cast(self.kf_out.ctypes.data, C.POINTER(self.orb.PoseSE3d)), p(self.pos_out, _f32p), p(self.erase, _u8p),
                p(self.chi2, f64p), *sem, C.byref(self.sres))
        rc = L.vsg_mappoints_read(self.mp.handle, self.npts, p(self.slots, _i32p), p(self.Xw, _f32p), None, None, None, None, None)
        if rc != 0:
            return rc
        rc = H.sg_host_side(self.cap, self.npts, p(self.slots, _i32p), p(self.Xw, _f32p), p(self.off, _i32p), p(self.okf, _i32p),
                            p(self.oidx, _i32p), self.K, p(self.kf_off, _i32p), p(self.kx, _f32p), p(self.ky, _f32p),
                            p(self.oct, _i32p), p(self.ur, _f32p), self.Tcw.ctypes.data, p(self.fixed, _u8p), self.cam.ctypes.data,
                            p(self.sig, _f32p), 8, 10, self.kf_out.ctypes.data, p(self.pos_out, _f32p), p(self.erase, _u8p),
                            p(self.chi2, f64p), *sem, C.addressof(self.sres))
        if rc != 0:
            return rc
        return L.vsg_mappoints_update(self.mp.handle, self.npts, p(self.slots, _i32p), p(self.pos_out, _f32p), None, None, None,
                                      None, None)

    def result(self, name, r):
        return LocalBA.result(self, name, r)[:6] + (
            self.plane_out.view(np.uint64).copy(), self.room_out.view(np.uint64).copy(), self.erase_plane.copy(),
            self.chi2k.view(np.uint64).copy(), self.chi2p.view(np.uint64).copy(), np.frombuffer(bytes(self.sres), np.uint8).copy())

    def facts(self, last):
        r = self.orb.SGraphLocalBaResult.from_buffer_copy(last["B"][11].tobytes())
        v = self.orb.LocalBaResult.from_buffer_copy(bytes(self.res))
        return {"optimised_keyframes": self.nk, "fixed_keyframes": self.nk, "points": self.npts, "edges": int(r.local.n_edges),
                "planes": self.n_planes, "rooms": self.n_rooms, "plane_observations": len(self.pkf),
                "plane_kf_edges": int(r.n_plane_kf), "plane_point_edges": int(r.n_plane_point), "rows": int(r.n_rows),
                "erased": int(r.local.n_erase), "erased_plane_observations": int(r.n_erase_plane), "features_per_keyframe": NFEAT,
                "iterations_run": int(r.local.iterations_run), "trials_run": int(r.local.trials_run),
                "stop_reason": int(r.local.stop_reason), "visual_call (iterations, trials)": (int(v.iterations_run), int(v.trials_run)),
                "every_call_equals_the_host_build": True,
                "host_side": "A = vsg_mappoints_read + the host build of csrc/vsg_sgraph_ba.h on one thread "
                             "(tools/resident_points_cpu.cpp) + vsg_mappoints_update; it is THIS header's build and NOT g2o (no "
                             "Eigen here): the same numeric Jacobians, no virtual calls, a DENSE reduced solve where g2o's is "
                             "sparse; B = vsg_mappoints_local_bundle_adjustment_sgraph; V = vsg_mappoints_local_bundle_adjustment "
                             "on the same scene without planes and rooms (B - V: the price of the semantic part)"}


class GlobalBA(LocalBA):
    """The visual part of Optimizer::BundleAdjustment behind GlobalBundleAdjustemnt on resident keyframes and map points:
    scenes of tests/lba_scenes.py with ONE fixed keyframe, keyframes padded to 1000 features.  "init": 1 + 1 keyframes, 300
    mono points, robust, 20 iterations.  "<K>": K keyframes, 15 K points of 8 observations, half stereo, 5 % outliers, not
    robust, 10 iterations.  write_store = 1 in both, so that the host side ends with vsg_mappoints_update."""
    SIZES = ("init", "50", "200", "500")
    TH, DEST = 0.0, "global_ba_latency.json"
    VARIANTS = ("A", "B", "A2", "B2")
    CALLS = {"init": (20, 200), "50": (5, 50), "100": (3, 20), "200": (1, 5), "500": (0, 3)}  # size -> (warm-up, timed calls)

    def __init__(self, orb, fr, size):
        import lba_scenes as ls
        if size == "init":
            nk, npts, self.robust, self.iterations = 2, 300, 1, 20
            scene = ls.make(7400, 1, 1, npts, 2, "mono")
        else:
            nk, self.robust, self.iterations = int(size), 0, 10
            npts = 15 * nk
            scene = ls.make(7400 + nk, nk - 1, 1, npts, 8, "mixed", outliers=0.05)
        self.setup(orb, scene, nk, npts)
        self.included, self.res = np.zeros(npts, np.uint8), orb.GlobalBaResult()

    def reset(self):
        self.mp.update(self.all, world_pos=self.pos0)
        self.kf_out[:], self.pos_out[:], self.included[:], self.chi2[:] = 0, 0, 9, -1.0
        C.memset(C.byref(self.res), 0, C.sizeof(self.res))

    def run(self, name, L, H, P):
        f64p = C.POINTER(C.c_double)
        if name.startswith("B"):
            return L.vsg_mappoints_global_bundle_adjustment(
                self.mp.handle, self.npts, p(self.slots, _i32p), p(self.off, _i32p), p(self.okf, _i32p), p(self.oidx, _i32p), self.K,
                self.handles, C.cast(self.Tcw.ctypes.data, C.POINTER(self.orb.PoseSE3)), p(self.fixed, _u8p),
                C.cast(self.cam.ctypes.data, C.POINTER(self.orb.BaCamera)), p(self.sig, _f32p), 8, self.iterations, self.robust, 1,
                None, C.cast(self.kf_out.ctypes.data, C.POINTER(self.orb.PoseSE3d)), p(self.pos_out, _f32p), p(self.included, _u8p),
                p(self.chi2, f64p), C.byref(self.res))
        rc = L.vsg_mappoints_read(self.mp.handle, self.npts, p(self.slots, _i32p), p(self.Xw, _f32p), None, None, None, None, None)
        if rc != 0:
            return rc
        rc = H.gb_host_side(self.cap, self.npts, p(self.slots, _i32p), p(self.Xw, _f32p), p(self.off, _i32p), p(self.okf, _i32p),
                            p(self.oidx, _i32p), self.K, p(self.kf_off, _i32p), p(self.kx, _f32p), p(self.ky, _f32p),
                            p(self.oct, _i32p), p(self.ur, _f32p), self.Tcw.ctypes.data, p(self.fixed, _u8p), self.cam.ctypes.data,
                            p(self.sig, _f32p), 8, self.iterations, self.robust, self.kf_out.ctypes.data, p(self.pos_out, _f32p),
                            p(self.included, _u8p), p(self.chi2, f64p), C.addressof(self.res))
        if rc != 0:
            return rc
        return L.vsg_mappoints_update(self.mp.handle, self.npts, p(self.slots, _i32p), p(self.pos_out, _f32p), None, None, None,
                                      None, None)

    def result(self, name, r):
        after = self.mp.read(self.slots)["world_pos"]
        return (r, self.kf_out.view(np.uint64).copy(), self.pos_out.copy(), after.reshape(-1).copy(), self.included.copy(),
                self.chi2.view(np.uint64).copy(), np.frombuffer(bytes(self.res), np.uint8).copy())

    def facts(self, last):
        r = self.orb.GlobalBaResult.from_buffer_copy(last["B"][6].tobytes())
        return {"keyframes": self.K, "optimised_keyframes": int(r.n_opt_kf), "fixed_keyframes": int(r.n_fixed_kf),
                "reduced_rows": 6 * int(r.n_opt_kf), "points": self.npts, "edges": int(r.n_edges), "mono": int(r.n_mono),
                "stereo": int(r.n_stereo), "robust": self.robust, "iterations": self.iterations, "features_per_keyframe": NFEAT,
                "iterations_run": int(r.iterations_run), "trials_run": int(r.trials_run), "stop_reason": int(r.stop_reason),
                "every_call_equals_the_host_build": True,
                "host_side": "A = vsg_mappoints_read + the host build of csrc/vsg_global_ba.h on one thread "
                             "(tools/resident_points_cpu.cpp) + vsg_mappoints_update; it is THIS header's build and NOT g2o (no "
                             "Eigen here).  Its DENSE reduced solve is dearer than g2o's sparse one for many keyframes, so the "
                             "larger sizes flatter the device; B = vsg_mappoints_global_bundle_adjustment"}


class Chain:
    """What the two chain cases add to their search's scene: a pose per call that stays within the search windows (a
    hundredth of a radian at most), the same pose as the solve's start, the solve's arrays, and the walk's rounds."""
    VARIANTS = ("A", "B", "A2", "B2")
    SIZES, DEST = (1000, 2000, 4000), "track_chain_latency.json"

    def chain_arrays(self):
        import pose_reference as pref
        self.pref = pref
        self.sig = (np.float32(1) / (self.sf * self.sf)).astype(np.float32)
        z = np.zeros
        self.fs, self.out, self.chi2 = z(NFEAT, np.int32), z(NFEAT, np.uint8), z(NFEAT, np.float32)
        self.pres, self.qt, self.ri, self.n_map = self.orb.PoseResult(), z(7), z(6, np.int32), C.c_int32(0)
        self.poses, self.rounds = {}, []

    def pose_at(self, k):
        k %= 50
        if k not in self.poses:
            a = 0.0002 * k
            Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
            po = self.pose
            R, t = Ry @ po["Rcw"].astype(np.float64), (Ry @ po["tcw"].astype(np.float64)).astype(np.float32)
            P = self.orb.FramePose.make(**self.fr.make_pose(R.astype(np.float32), t, po["fx"], po["fy"], po["cx"], po["cy"],
                                                            po["mbf"]))
            se3 = self.orb.PoseSE3()
            se3.q[:] = [float(v) for v in self.pref.q_from_matrix(R).astype(np.float32)]
            se3.t[:] = [float(v) for v in t]
            self.poses[k] = (P, se3)
        self.se3 = self.poses[k][1]
        return self.poses[k][0]

    def reset(self):
        self.tb[:], self.tm[:], self.fs[:], self.out[:], self.chi2[:], self.qt[:], self.ri[:] = 0, -1, -1, 7, -1.0, 0, 0

    def solve(self, L, P):
        """side A's second call: vsg_frame_pose_optimization on the slots the caller's loop made"""
        rc = L.vsg_frame_pose_optimization(self.F.handle, self.mp.handle, p(self.fs, _i32p), C.byref(self.se3), P.fx, P.fy, P.cx,
                                           P.cy, P.mbf, p(self.sig, _f32p), 8, -1, p(self.out, _u8p), p(self.chi2, _f32p),
                                           C.byref(self.pres))
        assert rc >= 0, rc
        self.take(self.pres)

    def take(self, pres):
        self.qt[:4], self.qt[4:] = pres.q[:], pres.t[:]
        self.ri[:3] = pres.n_initial, pres.n_bad, pres.rounds_run

    def result(self, name, r):
        return (r, self.fs.copy(), self.tm.copy(), self.out.copy(), self.chi2.view(np.uint32).copy(),
                self.qt.view(np.uint64).copy(), self.ri.copy())

    def chain_facts(self, last):
        b = last["B"]
        f = {"returned_last": int(b[0]), "edges_last": int(b[6][0]), "n_bad_last": int(b[6][1]), "rounds_run_last": int(b[6][2]),
             "caller_side": "A = the two existing calls of THIS library with the caller's loops between and after them "
                            "(tools/resident_points_cpu.cpp, one thread); B = the chain call"}
        if self.rounds:
            f["walk_rounds"] = {"min": int(min(self.rounds)), "median": float(np.median(self.rounds)),
                                "max": int(max(self.rounds))}
        return f


class Track(Chain, Last):
    """Tracking::TrackWithMotionModel: the scene of `last` with 1000 / 2000 / 4000 points (a quarter more last-frame
    features carry none).  A = vsg_frame_search_last_frame, the loop to mvpMapPoints, vsg_frame_pose_optimization, the
    discard loop; B = vsg_frame_track_with_motion_model.  (The walk's status is not part of vsg_track_result: no rounds.)"""
    TH = 7.0

    def __init__(self, orb, fr, n):
        Last.__init__(self, orb, fr, n)
        self.chain_arrays()
        self.tres = orb.TrackResult()

    def run(self, name, L, H, P):
        if name[0] == "B":
            rc = L.vsg_frame_track_with_motion_model(
                self.F.handle, self.L.handle, self.mp.handle, p(self.slots, _i32p), C.byref(P), C.byref(self.last_pose), self.mb,
                1, self.TH, p(self.sf, _f32p), 8, 1, C.byref(self.se3), p(self.sig, _f32p), -1, p(self.fs, _i32p),
                p(self.tm, _i32p), p(self.out, _u8p), p(self.chi2, _f32p), C.byref(self.tres))
            assert rc >= 0 and self.tres.optimized == 1 and self.tres.wide == 0, rc
            self.take(self.tres.pose)
            self.ri[3] = self.tres.n_matches_map
            return rc
        nm = Last.B(self, L, P)
        assert nm >= 20, nm  # the scene never needs the 2 * th search
        H.tk_slots_from_matches(NFEAT, p(self.tm, _i32p), p(self.slots, _i32p), None, p(self.fs, _i32p))
        self.solve(L, P)
        nm = H.tk_discard(NFEAT, nm, p(self.fs, _i32p), p(self.out, _u8p), p(self.observed, _u8p), C.byref(self.n_map))
        self.ri[3] = self.n_map.value
        return nm

    def facts(self, last):
        return dict(Last.facts(self, last), **self.chain_facts(last))


class TrackLocal(Chain, Local):
    """Tracking::TrackLocalMap: the scene of `local`; every third feature holds the point it was made from on entry and
    those points are flagged as seen.  A = the blocked array from the entry slots, vsg_frame_search_local_points, the loop
    to mvpMapPoints, vsg_frame_pose_optimization, the statistics loop; B = vsg_frame_track_local_map."""
    TH = 3.0

    def __init__(self, orb, fr, n):
        Local.__init__(self, orb, fr, n)
        self.chain_arrays()
        self.entry = np.where(np.arange(NFEAT) % 3 == 0, self.src, -1).astype(np.int32)
        self.skip = np.isin(self.slots, self.entry[self.entry >= 0]).astype(np.uint8)
        self.lres = orb.TrackLocalResult()

    def run(self, name, L, H, P):
        f = self.f
        if name[0] == "B":
            rc = L.vsg_frame_track_local_map(
                self.F.handle, self.mp.handle, self.n, p(self.slots, _i32p), p(self.skip, _u8p), C.byref(P), 0.5, self.TH,
                self.NNRATIO, 0, 0.0, p(self.sf, _f32p), 8, p(self.entry, _i32p), C.byref(self.se3), p(self.sig, _f32p), -1, 0,
                1, p(self.fs, _i32p), p(self.tm, _i32p), p(self.out, _u8p), p(self.chi2, _f32p), p(self.in_view, _u8p),
                p(self.px, _f32p), p(self.py, _f32p), C.byref(self.lres))
            self.take(self.lres.pose)
            self.ri[3], self.ri[4] = self.lres.n_to_match, self.lres.n_matches_searched
            self.rounds.append(self.lres.walk_rounds)
            return rc
        H.tk_blocked_from_slots(NFEAT, p(self.entry, _i32p), p(f["observed"], _u8p), p(self.tb, _u8p))
        nm = L.vsg_frame_search_local_points(
            self.F.handle, self.mp.handle, self.n, p(self.slots, _i32p), p(self.skip, _u8p), C.byref(P), 0.5, self.TH,
            self.NNRATIO, 0, 0.0, p(self.sf, _f32p), 8, p(self.tb, _u8p), p(self.tm, _i32p), p(self.in_view, _u8p),
            p(self.px, _f32p), p(self.py, _f32p), C.byref(self.ntm))
        assert nm >= 0, nm
        H.tk_slots_from_matches(NFEAT, p(self.tm, _i32p), p(self.slots, _i32p), p(self.entry, _i32p), p(self.fs, _i32p))
        self.solve(L, P)
        self.ri[3], self.ri[4] = self.ntm.value, nm
        return H.tk_local_stats(NFEAT, p(self.fs, _i32p), p(self.out, _u8p), p(f["observed"], _u8p), 0, 1)

    def facts(self, last):
        b = last["B"]
        return dict(self.chain_facts(last), n_to_match_last=int(b[6][3]), nmatches_last=int(b[6][4]),
                    entry_slots=int((self.entry >= 0).sum()))


class EssGraph:
    """Optimizer::OptimizeEssentialGraph on resident map points: a size is "<keyframes>:<fix_scale>".  One keyframe is fixed,
    every keyframe is joined to its five predecessors on the chain (about 6 edges per keyframe) and one loop edge closes the
    chain; the last three keyframes carry CorrectedSim3 (scale drift 1.3 without fix_scale, 1.0 with it); 10 map points per
    keyframe.  ITERATIONS = 3, not the reference's 20: the host side's dense solve takes seconds per trial at 438 keyframes, and
    three iterations are where the loop converges on these scenes (tests/eg_scenes.py)."""
    SIZES = ("50:0", "50:1", "200:0", "200:1", "438:0", "438:1")
    TH, DEST = 0.0, "essential_graph_latency.json"
    VARIANTS = ("A", "B", "A2", "B2")
    CALLS = {"50:0": (20, 200), "50:1": (20, 200), "200:0": (3, 50), "200:1": (3, 50), "438:0": (1, 5), "438:1": (1, 5)}
    ITERATIONS = 3

    def __init__(self, orb, fr, size):
        import eg_scenes as es
        nk, fix = (int(v) for v in size.split(":"))
        s = es.sized(8000 + nk, nk - 1, covis=5, scale=1.0 if fix else 1.3, fix_scale=fix, iterations=self.ITERATIONS, points_per_kf=10)
        self.orb, self.fix, self.K = orb, fix, nk
        f64 = np.float64
        self.Scw, self.nonc = np.ascontiguousarray(s["Scw"], f64), np.ascontiguousarray(s["nonc"], f64)
        self.has, self.fixed = np.ascontiguousarray(s["has"], np.uint8), np.ascontiguousarray(s["fixed"], np.uint8)
        self.ei = np.ascontiguousarray(np.append(s["ei"], nk - 1), np.int32)  # the loop edge: current -> keyframe 1
        self.ej = np.ascontiguousarray(np.append(s["ej"], 1), np.int32)
        self.el = np.ascontiguousarray(np.append(s["eloop"], 1), np.uint8)
        self.slots, self.ref = np.ascontiguousarray(s["slots"], np.int32), np.ascontiguousarray(s["point_ref"], np.int32)
        self.cap, self.npts, self.E = int(s["capacity"]), len(self.slots), len(self.ei)
        self.pos0 = np.ascontiguousarray(s["store_pos"], np.float32)
        self.all = np.arange(self.cap, dtype=np.int32)
        self.mp = orb.MapPoints(self.cap)
        self.Xw, self.pos_out = np.zeros((self.npts, 3), np.float32), np.zeros((self.npts, 3), np.float32)
        self.kf_out, self.chi2, self.res = np.zeros((nk, 8), f64), np.zeros(self.E, f64), orb.EssentialGraphResult()

    def pose_at(self, k):
        return None

    def reset(self):
        self.mp.update(self.all, world_pos=self.pos0)
        self.kf_out[:], self.pos_out[:], self.chi2[:] = 0, 0, -1.0
        C.memset(C.byref(self.res), 0, C.sizeof(self.res))

    def run(self, name, L, H, P):
        f64p, sp = C.POINTER(C.c_double), C.POINTER(self.orb.Sim3d)
        if name.startswith("B"):
            return L.vsg_mappoints_optimize_essential_graph(
                self.mp.handle, self.K, C.cast(self.Scw.ctypes.data, sp), C.cast(self.nonc.ctypes.data, sp), p(self.has, _u8p),
                p(self.fixed, _u8p), self.E, p(self.ei, _i32p), p(self.ej, _i32p), p(self.el, _u8p), self.fix, self.ITERATIONS, self.npts,
                p(self.slots, _i32p), p(self.ref, _i32p), C.cast(self.kf_out.ctypes.data, sp), p(self.pos_out, _f32p), p(self.chi2, f64p),
                C.byref(self.res))
        rc = L.vsg_mappoints_read(self.mp.handle, self.npts, p(self.slots, _i32p), p(self.Xw, _f32p), None, None, None, None, None)
        if rc != 0:
            return rc
        rc = H.eg_host_side(self.cap, self.K, self.Scw.ctypes.data, self.nonc.ctypes.data, p(self.has, _u8p), p(self.fixed, _u8p), self.E,
                            p(self.ei, _i32p), p(self.ej, _i32p), p(self.el, _u8p), self.fix, self.ITERATIONS, self.npts,
                            p(self.slots, _i32p), p(self.ref, _i32p), p(self.Xw, _f32p), self.kf_out.ctypes.data, p(self.pos_out, _f32p),
                            p(self.chi2, f64p), C.addressof(self.res))
        if rc != 0:
            return rc
        return L.vsg_mappoints_update(self.mp.handle, self.npts, p(self.slots, _i32p), p(self.pos_out, _f32p), None, None, None,
                                      None, None)

    def result(self, name, r):
        after = self.mp.read(self.all)["world_pos"]
        return (r, self.kf_out.view(np.uint64).copy(), self.pos_out.copy(), after.reshape(-1).copy(), self.chi2.view(np.uint64).copy(),
                np.frombuffer(bytes(self.res), np.uint8).copy())

    def facts(self, last):
        r = self.orb.EssentialGraphResult.from_buffer_copy(last["B"][5].tobytes())
        return {"keyframes": self.K, "optimised_keyframes": int(r.n_opt_kf), "rows": 7 * int(r.n_opt_kf), "edges": self.E,
                "points": self.npts, "fix_scale": self.fix, "iterations": self.ITERATIONS, "iterations_run": int(r.iterations_run),
                "trials_run": int(r.trials_run), "stop_reason": int(r.stop_reason), "chi2_initial": float(r.chi2_initial),
                "chi2_final": float(r.chi2_final), "every_call_equals_the_host_build": True,
                "host_side": "A = vsg_mappoints_read + the host build of csrc/vsg_essential_graph.h on one thread "
                             "(tools/resident_points_cpu.cpp) + vsg_mappoints_update; it is THIS header's build and NOT g2o (no "
                             "Eigen here).  Its DENSE solve is dearer than g2o's sparse one, which flatters the device at the "
                             "larger sizes; B = vsg_mappoints_optimize_essential_graph"}


CASES = {"track": Track, "track_local": TrackLocal, "local": Local, "last": Last, "keyframe": KeyFrame, "refresh": Refresh, "pose": Pose, "newpoints": NewPoints, "sim3": Sim3, "mlpnp": Mlpnp,
         "sim3opt": Sim3Opt, "localba": LocalBA, "sgraphba": SGraphBA, "globalba": GlobalBA, "twoview": TwoView, "essgraph": EssGraph}


def child(case, calls, sizes=None):
    import frustum_reference as fr
    from visual_sgraphs_amd import orb
    L, H, K = orb.load_library(), host_side(orb), CASES[case]
    out = {"calls": calls, "features": NFEAT, "th": K.TH, "sizes": {}}
    for n in sizes or K.SIZES:
        c = K(orb, fr, n)
        t = {k: [] for k in K.VARIANTS}
        last = {}
        warm, ncalls = getattr(K, "CALLS", {}).get(n, (20, calls))  # a case whose sizes differ by orders of magnitude says how many
        for k in range(ncalls + warm):
            P = c.pose_at(k)
            for name in K.VARIANTS:
                c.reset()
                t0 = time.perf_counter()
                r = c.run(name, L, H, P)
                dt = (time.perf_counter() - t0) * 1e6
                last[name] = c.result(name, r)
                assert last[name][0] >= 0, (name, last[name][0])
                if k >= warm:
                    t[name].append(dt)
            for name in getattr(K, "SAME", K.VARIANTS[1:]):  # the variants compute the same thing
                assert all(np.array_equal(a, b) for a, b in zip(last["A"], last[name])), name
        res = {k: stats(v) for k, v in t.items()}
        res.update(c.facts(last), timed_calls=ncalls, warm_up_calls=warm)
        res["a_vs_a_median_gap_us"] = round(abs(res["A"]["median_us"] - res["A2"]["median_us"]), 1)
        if "B2" in t:  # the resident call timed twice: its own repeat gap
            res["b_vs_b_median_gap_us"] = round(abs(res["B"]["median_us"] - res["B2"]["median_us"]), 1)
        # the resident call is "not slower" when its 10-90 % range does not lie wholly above the caller-side path's
        res["resident_not_slower"] = bool(res["B"]["p10_us"] <= max(res["A"]["p90_us"], res["A2"]["p90_us"]))
        res["resident_faster"] = bool(res["B"]["p90_us"] < min(res["A"]["p10_us"], res["A2"]["p10_us"]))
        # ... and its median gain counts when it is larger than the run's own A-vs-A gap
        if "V2" in t:  # the visual call on the same scene, twice: what the planes and rooms cost on the device
            res["semantic_part_median_us"] = round(res["B"]["median_us"] - res["V"]["median_us"], 1)
            res["v_vs_v_median_gap_us"] = round(abs(res["V"]["median_us"] - res["V2"]["median_us"]), 1)
        res["resident_median_gain_us"] = round(res["A"]["median_us"] - res["B"]["median_us"], 1)
        res["gain_exceeds_a_vs_a_gap"] = bool(res["resident_median_gain_us"] > res["a_vs_a_median_gap_us"])
        out["sizes"][str(n)] = res
    print(json.dumps(out))


def trace(case="local", size=None):
    import frustum_reference as fr
    from visual_sgraphs_amd import orb
    if case == "refresh":
        L, c = orb.load_library(), Refresh(orb, fr, 8000)
        for k in range(10):
            c.reset()
            assert c.B(L) == 0
        print({"n": 8000, "observations": len(c.kf), "best_not_first": int((c.best != 0).sum())})
        return
    if case == "localba":
        L, c = orb.load_library(), LocalBA(orb, fr, "20:3000")
        for k in range(5):
            c.reset()
            assert c.run("B", L, None, None) == 0
        print({"size": "20:3000", "calls": 5, "iterations_run": int(c.res.iterations_run), "trials_run": int(c.res.trials_run)})
        return
    if case == "sgraphba":
        L, c = orb.load_library(), SGraphBA(orb, fr, size or "20:3000:1")
        for k in range(5):
            c.reset()
            assert c.run("B", L, None, None) == 0
        print({"size": size or "20:3000:1", "calls": 5, "iterations_run": int(c.sres.local.iterations_run),
               "trials_run": int(c.sres.local.trials_run), "rows": int(c.sres.n_rows)})
        return
    if case == "essgraph":
        L, c = orb.load_library(), EssGraph(orb, fr, size or "200:0")
        for k in range(3):
            c.reset()
            assert c.run("B", L, None, None) == 0
        print({"size": size or "200:0", "calls": 3, "iterations_run": int(c.res.iterations_run), "trials_run": int(c.res.trials_run),
               "edges": c.E, "rows": 7 * int(c.res.n_opt_kf)})
        return
    if case == "globalba":  # a loop-closing problem through the new call and, where it accepts it, through the local call
        L, c = orb.load_library(), GlobalBA(orb, fr, size or "100")
        for k in range(3):
            c.reset()
            assert c.run("B", L, None, None) == 0
        out = {"size": size or "100", "calls_each": 3,
               "global (iterations, trials, optimised keyframes)": (int(c.res.iterations_run), int(c.res.trials_run), int(c.res.n_opt_kf))}
        if int(c.res.n_opt_kf) <= 128:  # the local call's cap
            c.erase, c.res = np.zeros(len(c.chi2), np.uint8), orb.LocalBaResult()
            for k in range(3):
                LocalBA.reset(c)
                assert LocalBA.run(c, "B", L, None, None) == 0
            out["local (iterations, trials)"] = (int(c.res.iterations_run), int(c.res.trials_run))
        print(out)
        return
    L, c = orb.load_library(), Local(orb, fr, 4000)
    for k in range(10):
        c.reset()
        assert c.B(L, c.pose_at(k)) >= 0
    print({"n": 4000, "nmatches": int((c.tm >= 0).sum()), "n_to_match": c.ntm.value})


def main(argv):
    if argv[0] == "child":
        return child(argv[1], int(argv[2]) if len(argv) > 2 else 200, argv[3].split(",") if len(argv) > 3 else None)
    if argv[1:2] == ["trace"]:
        return trace(argv[0], argv[2] if len(argv) > 2 else None)
    calls = int(argv[1]) if len(argv) > 1 else 200
    dest = Path(argv[2]) if len(argv) > 2 else ROOT / "profiles" / CASES[argv[0]].DEST
    r = subprocess.run([sys.executable, str(Path(__file__).resolve()), "child", argv[0], str(calls)], capture_output=True,
                       text=True, timeout=900)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        return r.returncode
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    dest.parent.mkdir(parents=True, exist_ok=True)
    if issubclass(CASES[argv[0]], Chain):  # both chain cases share one record, one key each
        both = json.loads(dest.read_text()) if dest.exists() else {}
        both[argv[0]] = rec
        rec = both
    dest.write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
