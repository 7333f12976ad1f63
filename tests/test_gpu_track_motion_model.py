"""GPU tests of Tracking::TrackWithMotionModel in one enqueue (vsg_frame_track_with_motion_model: projection, window
search, the ordered walk on the device, PoseOptimization) against the EXISTING two-call path of the library
(vsg_frame_search_last_frame, the caller's loop to mvpMapPoints, vsg_frame_pose_optimization, the discard loop), which the
library's own tests pin to the oracle and the restatements.  Equal bit for bit: train_match, nmatches, direction, the slots
after the discard, outlier, chi2, the pose, n_bad, rounds_run and the counts.  Scenes: tests/track_scenes.py."""
import ctypes as C

import numpy as np
import pytest

import projection_scenes as ps
import track_scenes as ts
from visual_sgraphs_amd import orb

pytestmark = pytest.mark.gpu
I32, U8 = np.int32, np.uint8


@pytest.fixture(scope="module")
def ex():
    return orb.ORBextractor(1000, 1.2, 8, 20, 7)


@pytest.fixture(scope="module", params=[False, True], ids=["gray", "rgbd"])
def scene(request, ex):
    return ts.Scene(ex, 3, request.param)


def both(s, th, **kw):
    want = s.two_calls_motion(th, **kw)
    got = s.chain_motion(th, **kw)
    ts.assert_same(got, want, ts.MOTION_KEYS, solved=bool(want["optimized"]))
    assert got["ret"] == want["n_matches"]
    return got, want


@pytest.mark.parametrize("th", [7, 15])
def test_equal_to_the_two_call_path(scene, th):
    got, want = both(scene, th)
    print(f"th {th}: nmatches {want['n_matches_searched']} edges {want['n_initial']} bad {want['n_bad']} "
          f"rounds {want['rounds_run']} map {want['n_matches_map']}")
    # conditions on the fixture: a real solve with outliers to discard and windows that collide
    assert want["optimized"] == 1 and want["wide"] == 0 and want["n_initial"] >= 100 and want["rounds_run"] == 4
    assert want["n_bad"] < want["n_initial"] and want["n_matches"] == want["n_matches_searched"] - want["n_bad"]
    if scene.ur is not None:  # a fifth of the depths disagree with mvuRight: stereo edges to discard
        assert want["n_bad"] > 0
    assert 0 < want["n_matches_map"] < want["n_matches"]
    assert (want["outlier"][want["train_match"] >= 0] == 0).all() and (want["outlier"][want["train_match"] < 0] == ts.FLAG).all()
    both(scene, th, check=False)
    both(scene, th, mono=True)


def test_past_1024_features_equal_to_the_two_call_path():
    """2000 features asked for, as the reference's KITTI settings do: the walk kernel's lanes go round their stride for the
    feature arrays and its edge compaction carries its base into a second chunk.  (Two points per keypoint: with three the
    last frame comes within 60 bytes of the walk's LDS cap.)"""
    s = ts.Scene(orb.ORBextractor(2000, 1.2, 8, 20, 7), 3, False, per_keypoint=2)
    got, want = both(s, 15)
    tm = want["train_match"]
    after_walk = np.where(tm >= 0, s.slots[np.maximum(tm, 0)], -1)  # the caller's loop, before the discard
    print(f"n {s.n} last {len(s.slots)} nmatches {want['n_matches_searched']} edges {want['n_initial']} "
          f"slots at >= 1024: {int((after_walk[1024:] >= 0).sum())} bad {want['n_bad']} rounds {want['rounds_run']}")
    assert s.n > 1024 and int((after_walk[1024:] >= 0).sum()) >= 50
    assert want["optimized"] == 1 and want["rounds_run"] == 4 and want["wide"] == 0
    assert got["n_initial"] == int((after_walk >= 0).sum())


def test_threshold_sweep_of_20_matches(scene):
    """15 .. 25 active last_slots around Tracking.cc:2958 / :2967: below 20 and lifted by the 2 * th search, below 20 and
    staying there, 20 or more at once."""
    s, th = scene, 1
    free = np.zeros(s.n, U8)
    narrow = s.F.SearchLastFrame(s.L, s.mp, s.slots, s.cp, s.lp, ps.MB, False, th, s.sf, free, False)[1]
    wide = s.F.SearchLastFrame(s.L, s.mp, s.slots, s.cp, s.lp, ps.MB, False, 2 * th, s.sf, free, False)[1]
    a, b = set(narrow[narrow >= 0].tolist()), set(wide[wide >= 0].tolist())
    in_both, wide_only = sorted(a & b), sorted(b - a)
    assert len(in_both) >= 25 and len(wide_only) >= 4, (len(in_both), len(wide_only))
    # the input pose as the existing solve hands it back when it has nothing to do (Optimizer.cc:1251)
    unsolved = s.F.pose_optimization(s.mp, np.full(s.n, -1, I32), s.q, s.t, s.camera, ts.SIG, np.zeros(s.n, U8))
    seen = set()
    for k in range(15, 26):
        for m in (0, 4):
            slots = np.full_like(s.slots, -1)
            active = in_both[:k - m] + wide_only[:m]
            slots[active] = s.slots[active]
            got, want = both(s, th, slots=slots, check=False)
            kind = "at once" if want["n_search"] >= 20 else "lifted" if want["n_matches_searched"] >= 20 else "stays below"
            seen.add(kind)
            assert got["wide"] == (0 if kind == "at once" else 1) and got["optimized"] == (0 if kind == "stays below" else 1)
            if kind == "stays below":
                assert (got["outlier"] == ts.FLAG).all() and got["n_matches"] == want["n_matches_searched"] < 20
                assert got["q"].tobytes() == unsolved["q"].tobytes() and got["t"].tobytes() == unsolved["t"].tobytes()
    assert seen == {"at once", "lifted", "stays below"}, seen


def test_hold_round_2_then_resume(scene):
    s = scene
    want = s.two_calls_motion(15, hold=2)
    assert want["held"] == 1
    removed = np.zeros(s.n, U8)
    removed[np.flatnonzero(want["feat_slots"] >= 0)[::7]] = 1
    want_r = s.F.pose_optimization_resume(want["outlier"], removed, want["chi2"])
    got = s.chain_motion(15, hold=2)
    ts.assert_same(got, want, ts.MOTION_KEYS)  # as after round 1: nothing discarded
    got_r = s.F.pose_optimization_resume(got["outlier"], removed, got["chi2"])
    ts.assert_same(got_r, want_r, ("ret", "held"), ("outlier", "chi2"))
    assert want_r["rounds_run"] == 4 and want_r["n_bad"] >= int(removed.sum())
    # nothing is held after a complete chain call, nor after a resume
    s.chain_motion(15)
    with pytest.raises(orb.VsgError) as e:
        s.F.pose_optimization_resume(got["outlier"], removed, got["chi2"])
    assert e.value.code == -6


def test_overflowing_lists_from_a_fresh_thread(ex):
    """A new host thread starts with room for 4 overflow entries per query: windows of th = 40 overflow it, the chain sees it
    in the walk kernel's status, solves nothing, and runs again with more room, as the existing path does."""
    s, th = ts.Scene(ex, 5, False), 40
    _, _, _, _, projected, u, v, _ = s.F.SearchLastFrame(s.L, s.mp, s.slots, s.cp, s.lp, ps.MB, False, th, s.sf,
                                                          np.zeros(s.n, U8))
    q = np.flatnonzero(projected)
    octv = s.lk["octave"][q].astype(I32)
    off, _ = s.F.GetFeaturesInArea(u[q], v[q], (np.float32(th) * s.sf[octv]).astype(np.float32), octv - 1, octv + 1)
    lens = np.diff(off)
    assert lens[lens > 16].sum() > 4 * len(s.slots), (int(lens[lens > 16].sum()), len(s.slots))  # the fixture overflows
    want = ts.in_thread(lambda: (s.two_calls_motion(th), s.two_calls_motion(7)))
    got = ts.in_thread(lambda: (s.chain_motion(th), s.chain_motion(7)))
    for g, w in zip(got, want):
        ts.assert_same(g, w, ts.MOTION_KEYS)
    # ... and the never-reset counter's base is right for whoever calls next on such a thread
    got = ts.in_thread(lambda: (s.chain_motion(th), s.two_calls_motion(th), s.chain_motion(th)))
    for g in got:
        ts.assert_same(g, want[0], ts.MOTION_KEYS)


def test_steady_state_allocates_nothing_and_empty_frames(scene):
    s = scene
    want = s.two_calls_motion(15)
    s.chain_motion(15)
    before = orb.thread_arena_growths()
    for _ in range(20):
        ts.assert_same(s.chain_motion(15), want, ts.MOTION_KEYS)
    assert orb.thread_arena_growths() == before
    # n = 0: an empty last frame, then an empty current frame
    e = orb.Frame(16)
    e.upload(np.zeros(0, orb.KP_DTYPE), np.zeros((0, 32), U8), ts.BOUNDS)
    out, chi2 = s.fresh()
    g = s.F.TrackWithMotionModel(e, s.mp, np.zeros(0, I32), s.cp, s.lp, ps.MB, False, 15, s.sf, s.q, s.t, ts.SIG, out, True,
                                 -1, chi2)
    assert g["ret"] == 0 and g["optimized"] == 0 and g["wide"] == 1 and g["n_search"] == 0
    assert (g["feat_slots"] == -1).all() and (g["train_match"] == -1).all() and (g["outlier"] == ts.FLAG).all()
    g = e.TrackWithMotionModel(s.L, s.mp, s.slots, s.cp, s.lp, ps.MB, False, 15, s.sf, s.q, s.t, ts.SIG, np.zeros(0, U8))
    assert g["ret"] == 0 and g["optimized"] == 0 and len(g["feat_slots"]) == 0
    ts.assert_same(s.chain_motion(15), want, ts.MOTION_KEYS)


def test_every_refusal_returns_its_code_and_leaves_the_thread_usable(scene):
    s, lib, n = scene, orb.load_library(), scene.n
    sf, sig = np.ascontiguousarray(s.sf, np.float32), np.ascontiguousarray(ts.SIG, np.float32)
    _f, _u8, _i32 = C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
    se3 = orb.Frame._se3(s.q, s.t)
    want = s.two_calls_motion(15)

    def raw(cur=s.F.handle, last=s.L.handle, mp=s.mp.handle, slots=s.slots, cp=s.cp, lp=s.lp, nlevels=8, scale=True, tcw=True,
            sigma=True, hold=-1, fs=True, out=True, res=True):
        sl = np.ascontiguousarray(slots, I32) if slots is not None else None
        f, o, r = np.full(n, -5, I32), np.full(n, ts.FLAG, U8), orb.TrackResult()
        r.n_search = -77
        rc = lib.vsg_frame_track_with_motion_model(
            cur, last, mp, sl.ctypes.data_as(_i32) if sl is not None else None, C.byref(cp) if cp is not None else None,
            C.byref(lp) if lp is not None else None, ps.MB, 0, 15.0, sf.ctypes.data_as(_f) if scale else None, nlevels, 1,
            C.byref(se3) if tcw else None, sig.ctypes.data_as(_f) if sigma else None, hold,
            f.ctypes.data_as(_i32) if fs else None, None, o.ctypes.data_as(_u8) if out else None, None,
            C.byref(r) if res else None)
        if rc < 0:  # an error writes nothing
            assert (f == -5).all() and (o == ts.FLAG).all() and r.n_search == -77
        return rc

    def after(code, rc):
        assert rc == code, (rc, code)
        ts.assert_same(s.chain_motion(15), want, ts.MOTION_KEYS)

    for kw in (dict(cur=None), dict(last=None), dict(mp=None), dict(cp=None), dict(lp=None), dict(scale=False),
               dict(slots=None), dict(tcw=False), dict(sigma=False), dict(fs=False), dict(out=False), dict(res=False),
               dict(hold=1), dict(hold=3), dict(nlevels=0), dict(nlevels=17), dict(nlevels=7)):
        after(-6, raw(**kw))
    bad = s.slots.copy()
    bad[np.flatnonzero(bad >= 0)[-1]] = s.mp.capacity
    after(-6, raw(slots=bad))
    half = len(s.lk) // 2
    stereo = orb.Frame(len(s.lk) + 1)
    stereo.upload(s.lk, np.zeros((len(s.lk), 32), U8), ts.BOUNDS, nleft=half)
    after(-3, raw(last=stereo.handle))
    after(-3, raw(cur=stereo.handle))
    assert raw() == want["n_matches"]
