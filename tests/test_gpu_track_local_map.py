"""GPU tests of Tracking::TrackLocalMap in one enqueue (vsg_frame_track_local_map: k_frustum, window search, the ordered
walk on the device with the entry slots, PoseOptimization, the statistics loop) against the EXISTING two-call path of the
library with the caller's loops between the calls: vsg_frame_search_local_points given the blocked array computed from the
entry slots, the loop from train_match to mvpMapPoints, vsg_frame_pose_optimization, and a numpy restatement of
Tracking.cc:3074-3095.  Equal bit for bit: train_match, nmatches, nToMatch, in_view, the projections, the slots, outlier,
chi2 (by its bytes), the pose, n_initial, n_bad, rounds_run, mnMatchesInliers and the return value.  Scenes:
tests/track_scenes.py (640 x 480, 1000 features, gray and RGB-D); the entry slots are what the motion-model call returned
on the same scene."""
import ctypes as C
import threading

import numpy as np
import pytest

import projection_scenes as ps
import track_scenes as ts
from visual_sgraphs_amd import orb

pytestmark = pytest.mark.gpu
F32, I32, U8 = np.float32, np.int32, np.uint8
NN = 0.8  # ORBmatcher matcher(0.8), Tracking.cc:3470
INTS = ("ret", "n_to_match", "n_matches_searched", "n_matches_inliers", "held", "n_initial", "n_bad", "rounds_run")
ARRAYS = ("train_match", "feat_slots", "outlier", "chi2", "in_view", "proj_x", "proj_y")
POPCOUNT = np.array([bin(v).count("1") for v in range(256)], np.int64)


def stats(fs, outlier, observed, only_tracking, drop_outliers):
    """Tracking.cc:3074-3095; observed is per SLOT."""
    fs = fs.copy()
    inliers = 0
    for i in np.flatnonzero(fs >= 0):
        if not outlier[i]:
            if only_tracking or observed[fs[i]]:
                inliers += 1
        elif drop_outliers:
            fs[i] = -1
    return inliers, fs


class Local:
    """A scene of tests/track_scenes.py with its local map: every point of the store in a seeded order, the entry slots of
    the motion-model call, and the points those features hold marked as seen (mnLastFrameSeen == mnId)."""

    def __init__(self, ex, seed, rgbd, per_keypoint=3):
        s = self.s = ts.Scene(ex, seed, rgbd, per_keypoint=per_keypoint)
        f2, self.desc, _ = ts.make_frame(ex, seed, rgbd)  # the scene's own frame once more, for its descriptors
        assert f2.kps.tobytes() == s.F.kps.tobytes()
        rng = np.random.default_rng(900 + seed)
        self.local = rng.permutation(s.mp.capacity).astype(I32)
        self.entry = s.chain_motion(15)["feat_slots"].copy()
        self.seen = np.isin(self.local, self.entry[self.entry >= 0]).astype(U8)

    def blocked(self, entry):
        return ((entry >= 0) & (self.s.observed[np.maximum(entry, 0)] != 0)).astype(U8)

    def two_calls(self, th, entry=None, local=None, skip="seen", pose=None, hold=-1, only_tracking=False, drop=False,
                  far=False, th_far=0.0):
        s = self.s
        entry = self.entry if entry is None else entry
        local = self.local if local is None else local
        skip = self.seen if isinstance(skip, str) else skip
        nm, tm, _, in_view, px, py, ntm = s.F.SearchLocalPoints(s.mp, pose or s.cp, th, NN, s.sf, self.blocked(entry),
                                                                slots=local, skip=skip, far_points=far, th_far_points=th_far)
        fs = np.where(tm >= 0, np.append(local, -1)[np.maximum(tm, 0)], entry).astype(I32)  # the caller's slot loop
        out, chi2 = s.fresh()
        r = s.F.pose_optimization(s.mp, fs, s.q, s.t, s.camera, ts.SIG, out, hold, chi2)
        r.update(train_match=tm, feat_slots=fs, in_view=in_view, proj_x=px, proj_y=py, n_to_match=ntm, n_matches_searched=nm,
                 n_matches_inliers=0, after_walk=fs)
        if not r["held"]:
            r["n_matches_inliers"], r["feat_slots"] = stats(fs, r["outlier"], s.observed, only_tracking, drop)
        r["ret"] = r["n_matches_inliers"]
        return r

    def chain(self, th, entry=None, local=None, skip="seen", pose=None, hold=-1, only_tracking=False, drop=False, far=False,
              th_far=0.0):
        s = self.s
        out, chi2 = s.fresh()
        return s.F.TrackLocalMap(s.mp, pose or s.cp, th, NN, s.sf, self.entry if entry is None else entry, s.q, s.t, ts.SIG,
                                 out, slots=self.local if local is None else local,
                                 skip=self.seen if isinstance(skip, str) else skip, far_points=far, th_far_points=th_far,
                                 hold_round=hold, only_tracking=only_tracking, drop_outliers=drop, chi2=chi2)

    def both(self, th, **kw):
        want, got = self.two_calls(th, **kw), self.chain(th, **kw)
        same(got, want)
        return got, want

    def best_candidates(self, th, skip):
        """Per searched query the nearest feature of its window, blocked or not (ORBmatcher.cc:62-120 without :88-90), and
        the windows' lengths; from isInFrustum, GetFeaturesInArea and the descriptors."""
        s = self.s
        v = s.F.isInFrustum(s.mp, s.cp, slots=self.local)
        q = np.flatnonzero((v["in_view"] != 0) & (skip == 0))
        lvl = v["scale_level"][q]
        r = np.where(v["view_cos"][q] > F32(0.998), F32(2.5), F32(4.0)).astype(F32)
        r = (r * F32(th) if th != 1 else r) * s.sf[lvl].astype(F32)
        off, idx = s.F.GetFeaturesInArea(v["proj_x"][q], v["proj_y"][q], r, lvl - 1, lvl)
        qdesc = ps.per_slot(s.fields, s.store_slots)["desc"][self.local[q]]
        best = np.full(len(q), -1, I32)
        for k in range(len(q)):
            c = idx[off[k]:off[k + 1]]
            if s.ur is not None and len(c):  # :92-97
                c = c[~((s.ur[c] > 0) & (np.abs(v["proj_xr"][q[k]] - s.ur[c]) > r[k]))]
            if len(c):
                best[k] = c[np.argmin(POPCOUNT[qdesc[k][None, :] ^ self.desc[c]].sum(1))]
        return best, np.diff(off)

    def away(self):
        """the scene's camera turned half round about its y axis: every point of the map lies behind it"""
        p = dict(self.s.pose)
        flip = np.diag([-1.0, 1.0, -1.0])
        p["Rcw"], p["tcw"] = (flip @ p["Rcw"].astype(np.float64)).astype(F32), (flip @ p["tcw"].astype(np.float64)).astype(F32)
        return orb.FramePose.make(**p)


def same(got, want):
    for k in INTS:
        assert got[k] == want[k], (k, got[k], want[k])
    for k in ARRAYS:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k
    assert got["q"].tobytes() == want["q"].tobytes() and got["t"].tobytes() == want["t"].tobytes()


@pytest.fixture(scope="module")
def ex():
    return orb.ORBextractor(1000, 1.2, 8, 20, 7)


@pytest.fixture(scope="module", params=[False, True], ids=["gray", "rgbd"])
def loc(request, ex):
    return Local(ex, 3, request.param)


@pytest.mark.parametrize("th", [1, 3])
def test_equal_to_the_two_call_path(loc, th):
    got, want = loc.both(th)
    s, entry, tm = loc.s, loc.entry, want["train_match"]
    blocked = loc.blocked(entry)
    best, _ = loc.best_candidates(th, loc.seen)
    new, overwritten = int((tm >= 0).sum()), int(((tm >= 0) & (entry >= 0)).sum())
    blocked_best = int(blocked[best[best >= 0]].sum())
    print(f"th {th}: entry {int((entry >= 0).sum())} to_match {want['n_to_match']} new {new} overwritten {overwritten} "
          f"blocked-best {blocked_best} edges {want['n_initial']} bad {want['n_bad']} rounds {want['rounds_run']} "
          f"inliers {want['n_matches_inliers']} walk rounds {got['walk_rounds']}")
    # conditions on the fixture, from the reference path's result
    assert want["n_to_match"] >= 500 and new >= 100 and overwritten >= 1 and blocked_best >= 1
    assert want["rounds_run"] == 4 and int((entry >= 0).sum()) >= 100
    if s.ur is not None:
        assert want["n_bad"] > 0
    assert not (blocked.astype(bool) & (tm >= 0)).any() and got["walk_rounds"] >= 1
    assert (want["outlier"][want["after_walk"] < 0] == ts.FLAG).all()


def test_past_1024_features_equal_to_the_two_call_path():
    """2000 features asked for, as the reference's KITTI settings do: the walk kernel's lanes go round their stride for the
    feature arrays, its prologue derives "blocked on entry" for features past the first 1024, and its edge compaction
    carries its base into a second chunk.  (Two points per keypoint: with three the call comes within 60 bytes of the
    walk's LDS cap.)"""
    loc = Local(orb.ORBextractor(2000, 1.2, 8, 20, 7), 3, False, per_keypoint=2)
    got, want = loc.both(3)
    s, after_walk = loc.s, want["after_walk"]
    print(f"n {s.n} local {len(loc.local)} entry {int((loc.entry >= 0).sum())} new {int((want['train_match'] >= 0).sum())} "
          f"edges {want['n_initial']} slots at >= 1024: {int((after_walk[1024:] >= 0).sum())} "
          f"claimed at >= 1024: {int((want['train_match'][1024:] >= 0).sum())} rounds {want['rounds_run']} "
          f"walk rounds {got['walk_rounds']}")
    assert s.n > 1024 and int((after_walk[1024:] >= 0).sum()) >= 50
    assert want["held"] == 0 and want["rounds_run"] == 4  # the solve ran all its rounds
    assert int((want["train_match"][1024:] >= 0).sum()) >= 1 and int((loc.entry[1024:] >= 0).sum()) >= 1
    assert got["n_initial"] == int((after_walk >= 0).sum())


@pytest.mark.parametrize("only_tracking", [0, 1])
@pytest.mark.parametrize("drop", [0, 1])
def test_statistics_and_the_stereo_drop(loc, only_tracking, drop):
    got, want = loc.both(3, only_tracking=bool(only_tracking), drop=bool(drop))
    n_out = int(((want["after_walk"] >= 0) & (want["outlier"] == 1)).sum())
    assert int((want["after_walk"] != want["feat_slots"]).sum()) == (n_out if drop else 0)
    assert want["n_matches_inliers"] > 0
    if loc.s.ur is not None:
        assert n_out > 0
        if drop:  # :3093 drops the point and leaves mvbOutlier set
            gone = want["after_walk"] != got["feat_slots"]
            assert (got["outlier"][gone] == 1).all() and (got["feat_slots"][gone] == -1).all()


def test_only_tracking_counts_the_unobserved_inliers_too(loc):
    a, b = loc.chain(3, only_tracking=False), loc.chain(3, only_tracking=True)
    assert a["n_matches_inliers"] < b["n_matches_inliers"]  # a fifth of the store is not observed
    assert a["feat_slots"].tobytes() == b["feat_slots"].tobytes()


def test_far_points_remove_part_of_the_in_view_points(loc):
    v = loc.s.F.isInFrustum(loc.s.mp, loc.s.cp, slots=loc.local)
    depth = v["depth"][(v["in_view"] != 0) & (loc.seen == 0)]
    th_far = float(np.median(depth))
    got, want = loc.both(3, far=True, th_far=th_far)
    near = loc.two_calls(3)
    assert 0 < want["n_matches_searched"] < near["n_matches_searched"] and want["n_to_match"] == near["n_to_match"]


def test_skip_set_for_half_of_the_points(loc):
    skip = (np.arange(len(loc.local)) % 2).astype(U8)
    got, want = loc.both(3, skip=skip)
    assert (want["in_view"][skip == 1] == 0).all() and (want["proj_x"][skip == 1] == -1).all()
    assert 0 < want["n_to_match"] and want["n_matches_searched"] > 0
    none, _ = loc.both(3, skip=None)
    assert none["n_to_match"] > want["n_to_match"]


def test_nothing_to_search_is_pose_optimization_on_the_entry_slots(loc):
    s = loc.s
    out, chi2 = s.fresh()
    p = s.F.pose_optimization(s.mp, loc.entry, s.q, s.t, s.camera, ts.SIG, out, -1, chi2)
    assert p["rounds_run"] == 4 and p["n_initial"] == int((loc.entry >= 0).sum())
    for kw in (dict(local=np.zeros(0, I32), skip=None), dict(skip=np.ones(len(loc.local), U8)), dict(pose=loc.away())):
        got, want = loc.both(3, **kw)
        assert want["n_to_match"] == 0 and want["n_matches_searched"] == 0 and (want["train_match"] == -1).all()
        for k in ("n_initial", "n_bad", "rounds_run"):
            assert got[k] == p[k]
        assert got["q"].tobytes() == p["q"].tobytes() and got["t"].tobytes() == p["t"].tobytes()
        assert got["outlier"].tobytes() == p["outlier"].tobytes() and got["chi2"].tobytes() == p["chi2"].tobytes()
        assert got["feat_slots"].tobytes() == loc.entry.tobytes()


@pytest.mark.parametrize("edges", [2, 3])
def test_two_and_three_edges_around_optimizer_1251(loc, edges):
    entry = np.full_like(loc.entry, -1)
    keep = np.flatnonzero(loc.entry >= 0)[5:5 + edges]
    entry[keep] = loc.entry[keep]
    got, want = loc.both(3, entry=entry, pose=loc.away())
    assert want["n_initial"] == edges and want["n_matches_searched"] == 0
    assert want["rounds_run"] == (0 if edges < 3 else 1)  # fewer than 10 edges end the loop after one round (:1440)
    assert (got["outlier"][keep] != ts.FLAG).all() and (np.delete(got["outlier"], keep) == ts.FLAG).all()
    if edges < 3:
        assert (got["outlier"][keep] == 0).all()


def test_hold_round_2_then_resume(loc):
    s = loc.s
    want = loc.two_calls(3, hold=2, drop=True)
    assert want["held"] == 1 and want["ret"] == 0
    removed = np.zeros(s.n, U8)
    removed[np.flatnonzero(want["feat_slots"] >= 0)[::7]] = 1
    want_r = s.F.pose_optimization_resume(want["outlier"], removed, want["chi2"])
    got = loc.chain(3, hold=2, drop=True)
    same(got, want)  # as after round 1: no statistics, nothing dropped
    got_r = s.F.pose_optimization_resume(got["outlier"], removed, got["chi2"])
    ts.assert_same(got_r, want_r, ("ret", "held"), ("outlier", "chi2"))
    assert want_r["rounds_run"] == 4 and want_r["n_bad"] >= int(removed.sum())
    loc.chain(3)  # nothing is held after a complete chain call
    with pytest.raises(orb.VsgError) as e:
        s.F.pose_optimization_resume(got["outlier"], removed, got["chi2"])
    assert e.value.code == -6


def test_overflowing_lists_from_a_fresh_thread(ex):
    """A new host thread starts with room for 4 overflow entries per query: windows of th = 15 overflow it, the chain sees
    it in the walk kernel's status, solves nothing, and runs again with more room, as the existing path does."""
    loc, th = Local(ex, 5, False), 15
    _, lens = loc.best_candidates(th, loc.seen)
    assert lens[lens > 16].sum() > 4 * len(loc.local), (int(lens[lens > 16].sum()), len(loc.local))  # the fixture overflows
    want = ts.in_thread(lambda: (loc.two_calls(th), loc.two_calls(3)))
    got = ts.in_thread(lambda: (loc.chain(th), loc.chain(3)))
    for g, w in zip(got, want):
        same(g, w)
    # ... and the never-reset counter's base is right for whoever calls next on such a thread
    got = ts.in_thread(lambda: (loc.chain(th), loc.two_calls(th), loc.chain(th)))
    for g in got:
        same(g, want[0])


def test_steady_state_allocates_nothing(loc):
    want = loc.two_calls(3)
    loc.chain(3)
    before = orb.thread_arena_growths()
    for _ in range(20):
        same(loc.chain(3), want)
    assert orb.thread_arena_growths() == before


def test_a_frame_without_features_returns_zero(loc):
    s = loc.s
    e = orb.Frame(16)
    e.upload(np.zeros(0, orb.KP_DTYPE), np.zeros((0, 32), U8), ts.BOUNDS)
    g = e.TrackLocalMap(s.mp, s.cp, 3, NN, s.sf, np.zeros(0, I32), s.q, s.t, ts.SIG, np.zeros(0, U8), slots=loc.local)
    assert g["ret"] == 0 and g["n_matches_inliers"] == 0 and g["n_initial"] == 0 and len(g["feat_slots"]) == 0


def test_both_chain_calls_from_two_host_threads_at_once(ex, loc):
    """TrackLocalMap on one frame and TrackWithMotionModel on another from two host threads at the same time: every
    result equals the single-thread one; each thread releases its stream and arenas before it ends."""
    other = ts.Scene(ex, 4, False)
    want_local, want_motion = loc.chain(3), other.chain_motion(15)
    same(want_local, loc.two_calls(3))
    gate, box = threading.Barrier(2), {}

    def run(name, fn):
        try:
            gate.wait(timeout=60)
            box[name] = ("ok", [fn() for _ in range(10)])
        except BaseException as e:  # noqa: BLE001
            box[name] = ("err", e)
        finally:
            orb.load_library().vsg_thread_release()

    threads = [threading.Thread(target=run, args=("local", lambda: loc.chain(3))),
               threading.Thread(target=run, args=("motion", lambda: other.chain_motion(15)))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for name in ("local", "motion"):
        if box[name][0] == "err":
            raise box[name][1]
    for g in box["local"][1]:
        same(g, want_local)
    for g in box["motion"][1]:
        ts.assert_same(g, want_motion, ts.MOTION_KEYS)


def test_every_refusal_returns_its_code_and_leaves_the_thread_usable(loc):
    s, lib, nf = loc.s, orb.load_library(), loc.s.n
    sf, sig = np.ascontiguousarray(s.sf, F32), np.ascontiguousarray(ts.SIG, F32)
    _f, _u8, _i32 = C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
    se3 = orb.Frame._se3(s.q, s.t)
    want = loc.two_calls(3)
    ptr = lambda a, t: a.ctypes.data_as(t) if a is not None else None

    def raw(F=s.F.handle, mp=s.mp.handle, local=loc.local, n=None, cp=s.cp, nlevels=8, scale=True, entry=loc.entry,
            tcw=True, sigma=True, hold=-1, fs=True, out=True, res=True):
        sl = np.ascontiguousarray(local, I32) if local is not None else None
        n = len(sl) if n is None else n
        fin = np.ascontiguousarray(entry, I32) if entry is not None else None
        sk = np.ascontiguousarray(np.resize(loc.seen, max(n, 1)), U8)
        f, tm, o, c2 = np.full(nf, -5, I32), np.full(nf, -5, I32), np.full(nf, ts.FLAG, U8), np.full(nf, -3, F32)
        iv, px, py = np.full(max(n, 1), 9, U8), np.full(max(n, 1), -3, F32), np.full(max(n, 1), -3, F32)
        r = orb.TrackLocalResult()
        r.n_to_match = -77
        rc = lib.vsg_frame_track_local_map(
            F, mp, n, ptr(sl, _i32), ptr(sk, _u8), C.byref(cp) if cp is not None else None, 0.5, 3.0, NN, 0, 0.0,
            ptr(sf, _f) if scale else None, nlevels, ptr(fin, _i32), C.byref(se3) if tcw else None,
            ptr(sig, _f) if sigma else None, hold, 0, 0, ptr(f, _i32) if fs else None, ptr(tm, _i32),
            ptr(o, _u8) if out else None, ptr(c2, _f), ptr(iv, _u8), ptr(px, _f), ptr(py, _f), C.byref(r) if res else None)
        if rc < 0:  # an error writes nothing
            assert (f == -5).all() and (tm == -5).all() and (o == ts.FLAG).all() and (c2 == -3).all()
            assert (iv == 9).all() and (px == -3).all() and (py == -3).all() and r.n_to_match == -77
        return rc

    def after(code, rc):
        assert rc == code, (rc, code)
        same(loc.chain(3), want)

    for kw in (dict(F=None), dict(mp=None), dict(cp=None), dict(scale=False), dict(entry=None), dict(tcw=False),
               dict(sigma=False), dict(fs=False), dict(out=False), dict(res=False), dict(hold=1), dict(hold=3),
               dict(nlevels=0), dict(nlevels=17), dict(nlevels=7), dict(n=-1)):
        after(-6, raw(**kw))
    bad = loc.local.copy()
    bad[-1] = s.mp.capacity
    after(-6, raw(local=bad))
    bad[-1] = -1
    after(-6, raw(local=bad))
    bad = loc.entry.copy()
    bad[np.flatnonzero(bad < 0)[0]] = s.mp.capacity
    after(-6, raw(entry=bad))
    # a pyramid of 4 levels for a frame whose features reach octave 7: EVERY feature's octave is checked
    assert s.F.kps["octave"].max() >= 4
    low = dict(s.pose, n_levels=4)
    after(-6, raw(cp=orb.FramePose.make(**low), nlevels=4))
    stereo = orb.Frame(len(s.lk) + 1)
    stereo.upload(s.lk, np.zeros((len(s.lk), 32), U8), ts.BOUNDS, nleft=len(s.lk) // 2)
    after(-3, raw(F=stereo.handle))
    # 2 * features + n above the walk's LDS cap: a long slot list (slots may repeat), refused before anything is enqueued
    long_list = np.resize(loc.local, 16000)
    assert 2 * nf + len(long_list) > 16000
    after(-2, raw(local=long_list))
    assert raw() == want["ret"]
