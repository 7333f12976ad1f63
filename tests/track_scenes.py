"""Scenes and the caller-side reference path for the GPU tests of the chain call
(tests/test_gpu_track_motion_model.py).  The scenes are those of tests/projection_scenes.py: a real extracted current frame (gray or RGB-D), map points made from its own keypoints `per_keypoint` times each (3: the
windows collide), a last frame that observes them.  The reference is the EXISTING two-call path of the library with the
caller's loops between the calls, as Tracking.cc has them."""
import threading

import numpy as np

import pose_reference as pref
import pose_scenes as pose_sc
import projection_scenes as ps
import rgbd_reference as rr
from visual_sgraphs_amd import orb, synth

F32, I32, U8 = np.float32, np.int32, np.uint8
W, H = 640, 480
BOUNDS = (0.0, 0.0, float(W), float(H))
SIG = pose_sc.INV_SIGMA2
FLAG, CHI2 = 7, -1.0  # sentinels: entries of features without a map point keep them


def make_frame(ex, seed, rgbd):
    img = synth.sequence_frame(W, H, seed, 0)
    f = orb.Frame(ex.capacity(H, W))
    if rgbd:
        plane = rr.depth_plane(30 + seed, H, W, np.uint16)
        _, _, d, ur, _ = f.extract_into_rgbd(ex, img, plane, BOUNDS, None, None, F32(0.001), ps.CAM[6])
        assert (ur > 0).sum() > 100
    else:
        _, _, d = f.extract_into(ex, img, BOUNDS)
        ur = None
    assert len(f.kps) > 500
    return f, d, ur


def in_thread(fn):
    """run fn on a freshly started host thread (its own stream, arena and candidate-stride hint); re-raise what it raised"""
    box = []

    def run():
        try:
            box.append(("ok", fn()))
        except BaseException as e:  # noqa: BLE001
            box.append(("err", e))
        finally:
            orb.load_library().vsg_thread_release()
    t = threading.Thread(target=run)
    t.start()
    t.join()
    if box[0][0] == "err":
        raise box[0][1]
    return box[0][1]


class Scene:
    def __init__(self, ex, seed, rgbd, per_keypoint=3, n_other=300):
        self.F, desc, self.ur = make_frame(ex, seed, rgbd)
        self.n = len(self.F.kps)
        self.pose = ps.current_pose(seed)
        self.fields, src = ps.map_points(self.F.kps, desc, self.ur, self.pose, 100 + seed, per_keypoint, n_other=n_other)
        self.last_pose = ps.last_pose_of(self.pose, 0.0, 200 + seed)
        self.L, self.lk, self.slots, self.store_slots = ps.last_frame(self.F.kps, self.fields, src, self.last_pose, BOUNDS,
                                                                      300 + seed)
        self.mp = ps.store_of(self.fields, self.store_slots)
        self.observed = ps.per_slot(self.fields, self.store_slots)["observed"]
        self.sf = ex.GetScaleFactors()
        self.cp, self.lp = orb.FramePose.make(**self.pose), orb.FramePose.make(**self.last_pose)
        self.q = pref.q_from_matrix(self.pose["Rcw"].astype(np.float64)).astype(F32)
        self.t = self.pose["tcw"].astype(F32)
        self.camera = tuple(self.pose[k] for k in ("fx", "fy", "cx", "cy", "mbf"))

    def fresh(self):
        return np.full(self.n, FLAG, U8), np.full(self.n, CHI2, F32)

    # ---- TrackWithMotionModel
    def chain_motion(self, th, slots=None, check=True, hold=-1, mono=False):
        out, chi2 = self.fresh()
        return self.F.TrackWithMotionModel(self.L, self.mp, self.slots if slots is None else slots, self.cp, self.lp, ps.MB,
                                           mono, th, self.sf, self.q, self.t, SIG, out, check, hold, chi2)

    def two_calls_motion(self, th, slots=None, check=True, hold=-1, mono=False):
        """Tracking.cc:2945-3005 on the existing calls: the search, the retry with 2 * th, the loop from train_match to
        mvpMapPoints, PoseOptimization, the discard loop."""
        slots = self.slots if slots is None else slots
        free = np.zeros(self.n, U8)
        nm, tm, _, direction, *_ = self.F.SearchLastFrame(self.L, self.mp, slots, self.cp, self.lp, ps.MB, mono, th,
                                                          self.sf, free, check)
        r = dict(n_search=nm, wide=0, direction=direction)
        if nm < 20:
            nm, tm, _, direction, *_ = self.F.SearchLastFrame(self.L, self.mp, slots, self.cp, self.lp, ps.MB, mono,
                                                              2 * th, self.sf, free, check)
            r["wide"] = 1
        fs = np.where(tm >= 0, slots[np.maximum(tm, 0)], -1).astype(I32)
        out, chi2 = self.fresh()
        r.update(n_matches_searched=nm, train_match=tm, feat_slots=fs, outlier=out, chi2=chi2, optimized=0, n_matches=nm,
                 n_matches_map=0, held=0)
        if nm < 20:
            return r
        p = self.F.pose_optimization(self.mp, fs, self.q, self.t, self.camera, SIG, out, hold, chi2)
        r.update(p, optimized=1)
        if p["held"]:
            return r
        return self.discard(r, nm)

    def discard(self, r, nm):
        fs, out = r["feat_slots"].copy(), r["outlier"].copy()
        n_map = 0
        for i in np.flatnonzero(fs >= 0):
            if out[i]:
                fs[i], out[i], nm = -1, 0, nm - 1
            elif self.observed[fs[i]]:
                n_map += 1
        r.update(feat_slots=fs, outlier=out, n_matches=nm, n_matches_map=n_map)
        return r


MOTION_KEYS = ("n_search", "wide", "n_matches_searched", "optimized", "n_matches", "n_matches_map", "direction", "held")
POSE_KEYS = ("n_initial", "n_bad", "rounds_run")
ARRAYS = ("train_match", "feat_slots", "outlier", "chi2")


def assert_same(got, want, keys, arrays=ARRAYS, solved=True):
    """Bit for bit: the counts, the arrays (chi2 by its bytes: NaN equals NaN), and the solve's result where it ran."""
    for k in keys:
        assert got[k] == want[k], (k, got[k], want[k])
    for k in arrays:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k
    if solved:
        for k in POSE_KEYS:
            assert got[k] == want[k], (k, got[k], want[k])
        assert got["q"].tobytes() == want["q"].tobytes() and got["t"].tobytes() == want["t"].tobytes()
