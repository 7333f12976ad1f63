"""GPU tests of SearchByProjection(CurrentFrame, LastFrame, th, bMono) on resident map points
(vsg_frame_search_last_frame) against the EXISTING vsg_frame_search_by_projection_last (oracle-checked by
tests/test_gpu_frame.py) fed with tests/projection_reference.py's arrays: nmatches, train_match (mapped back through the
index map) and train_blocked identical; direction equal; projected, u, v, ur bit-equal to the restatement.  The current
frame is a real extracted one (gray and RGB-D, so the mvuRight gate is live); the map points are its keypoints
un-projected through its pose (tests/projection_scenes.py), the last frame observes them from a pose placed along the
optical axis."""
import ctypes as C
import threading

import numpy as np
import pytest

import projection_reference as pr
import projection_scenes as ps
import rgbd_reference as rr
from visual_sgraphs_amd import orb, synth

pytestmark = pytest.mark.gpu
W, H = 640, 480
BOUNDS = (0.0, 0.0, float(W), float(H))


@pytest.fixture(scope="module")
def ex():
    return orb.ORBextractor(1000, 1.2, 8, 20, 7)


def make_frame(ex, seed, rgbd):
    img = synth.sequence_frame(W, H, seed, 0)
    f = orb.Frame(ex.capacity(H, W))
    if rgbd:
        plane = rr.depth_plane(30 + seed, H, W, np.uint16)
        _, _, d, ur, _ = f.extract_into_rgbd(ex, img, plane, BOUNDS, None, None, np.float32(0.001), ps.CAM[6])
        assert (ur > 0).sum() > 100
    else:
        _, _, d = f.extract_into(ex, img, BOUNDS)
        ur = None
    assert len(f.kps) > 500
    return f, d, ur


class Scene:
    def __init__(self, ex, seed, rgbd, along=0.0, per_keypoint=1, capacity_factor=None, extra=0.25, outliers=0.10,
                 n_other=300):
        self.F, desc, ur = make_frame(ex, seed, rgbd)
        self.pose = ps.current_pose(seed)
        self.fields, src = ps.map_points(self.F.kps, desc, ur, self.pose, 100 + seed, per_keypoint,
                                            n_other=n_other)
        self.cap = int(capacity_factor * len(src)) + 5 if capacity_factor else None
        self.last_pose = ps.last_pose_of(self.pose, along, 200 + seed)
        self.L, self.lk, self.slots, self.store_slots = ps.last_frame(self.F.kps, self.fields, src, self.last_pose, BOUNDS,
                                                                      300 + seed, extra, outliers, self.cap)
        self.mp = ps.store_of(self.fields, self.store_slots, self.cap)
        self.by_slot = ps.per_slot(self.fields, self.store_slots, self.cap)
        self.sf = ex.GetScaleFactors()
        self.cp, self.lp = orb.FramePose.make(**self.pose), orb.FramePose.make(**self.last_pose)

    def reference(self, th, mono, check, blocked, min_match=0.10):
        """(want, ref, direction) of the existing path on the restatement's arrays, with the conditions on the fixture."""
        active = self.slots >= 0
        P = self.by_slot["world_pos"][np.maximum(self.slots, 0)]
        ref = pr.project_last_points(self.pose, BOUNDS, P, active)
        a = pr.last_frame_fields(ref, self.slots, self.lk, self.by_slot["desc"], self.by_slot["observed"])
        direction = pr.motion_direction(self.pose, self.last_pose, ps.MB, mono)
        want = self.F.SearchByProjection_Last(a["desc"], a["observed"], a["u"], a["v"], a["ur"], a["last_octave"],
                                              a["last_angle"], th, direction, self.sf, check, blocked)
        want = (want[0], pr.map_back(want[1], a["index"]), want[2])
        n_proj = int(ref["valid"].sum())
        print(f"last N={len(self.slots)} slots {int(active.sum())} projected {n_proj} nmatches {want[0]} th {th} "
              f"direction {direction} check {check}")
        if min_match is not None:  # conditions on the fixture and the existing path, not on the code under test
            assert active.mean() >= 0.60, active.mean()
            assert n_proj >= 0.5 * active.sum(), (n_proj, int(active.sum()))
            assert want[0] >= min_match * n_proj, (want[0], n_proj)
        return want, ref, direction

    def search(self, th, mono, check, blocked):
        return self.F.SearchLastFrame(self.L, self.mp, self.slots, self.cp, self.lp, ps.MB, mono, th, self.sf, blocked,
                                      check)

    def compare(self, th, mono=False, check=True, blocked=None, min_match=0.10):
        blocked = np.zeros(len(self.F.kps), np.uint8) if blocked is None else blocked
        want, ref, direction = self.reference(th, mono, check, blocked, min_match)
        got = self.search(th, mono, check, blocked)
        assert_equal(got, want, ref, direction)
        return want, got, ref, direction


def assert_equal(got, want, ref, direction):
    assert got[0] == want[0]
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert got[3] == direction
    assert np.array_equal(got[4], ref["valid"])
    for a, k in ((got[5], "u"), (got[6], "v"), (got[7], "ur")):
        assert a.dtype == ref[k].dtype and a.tobytes() == ref[k].tobytes(), k  # bit patterns: NaN equals NaN


@pytest.mark.parametrize("rgbd", [False, True], ids=["gray", "rgbd"])
@pytest.mark.parametrize("th", [7, 15, 30])
def test_equal_to_search_by_projection_last(ex, rgbd, th):
    s = Scene(ex, 3, rgbd)
    want, got, _, direction = s.compare(th)
    assert direction == 0
    if rgbd and th == 7:
        # the gate is live (the narrow window is the one a wrong depth leaves): without mvuRight the same points match differently
        g = Scene(ex, 3, False)
        g.L, g.mp, g.slots = s.L, s.mp, s.slots
        g.cp, g.lp = s.cp, s.lp
        other = g.search(th, False, True, np.zeros(len(g.F.kps), np.uint8))
        assert not np.array_equal(other[1], got[1])
    # train_blocked pre-set on a tenth of the features
    rng = np.random.default_rng(th)
    s.compare(th, blocked=(rng.random(len(s.F.kps)) < 0.1).astype(np.uint8))
    # the rotation filter off
    off, _, _, _ = s.compare(th, check=False)
    assert off[0] >= want[0]


@pytest.mark.parametrize("rgbd", [False, True], ids=["gray", "rgbd"])
@pytest.mark.parametrize("along,expect", [(2 * ps.MB, 1), (-2 * ps.MB, 2), (0.0, 0)], ids=["forward", "backward", "neither"])
def test_direction_selects_the_level_window(ex, rgbd, along, expect):
    s = Scene(ex, 4, rgbd, along)
    want, got, _, direction = s.compare(15)
    assert direction == expect
    # bMono switches both directions off: the window is +-1 again
    wm, gm, _, dm = s.compare(15, mono=True)
    assert dm == 0
    if expect:
        assert not np.array_equal(gm[1], got[1])
    s.compare(15, check=False)


def test_rotation_filter_drops_a_match_somewhere(ex):
    """Condition on the fixtures (the existing path alone): the three-maxima filter removes a match in at least one of the
    parametrisations above."""
    s = Scene(ex, 3, False)
    blocked = np.zeros(len(s.F.kps), np.uint8)
    pairs = [(s.reference(th, False, True, blocked)[0][0], s.reference(th, False, False, blocked)[0][0]) for th in (7, 15, 30)]
    assert any(on < off for on, off in pairs), pairs


def test_store_larger_than_the_slot_list_and_retry_with_twice_th(ex):
    s = Scene(ex, 5, True, capacity_factor=2.0)
    assert s.mp.capacity > len(s.store_slots) and not np.array_equal(s.store_slots, np.arange(len(s.store_slots)))
    base = Scene(ex, 5, True)
    w0, _, _, _ = base.compare(7)
    w1, g1, _, _ = s.compare(7)
    assert w0[0] == w1[0] and np.array_equal(w0[1], w1[1])  # train_match holds last-frame features either way
    # Tracking.cc:2956-2961: th, then 2 * th on the same thread, nothing but th changes
    w2, g2, _, _ = s.compare(14)
    assert not np.array_equal(g1[1], g2[1])
    s.compare(7)


def test_empty_all_outliers_and_more_than_4096_features(ex):
    s = Scene(ex, 6, False, per_keypoint=5)
    assert s.L.N > 4096
    s.compare(7)
    # every slot -1: nothing is projected, nothing matches
    keep = s.slots.copy()
    s.slots = np.full_like(keep, -1)
    want, got, ref, _ = s.compare(7, min_match=None)
    assert got[0] == 0 and (got[1] == -1).all() and not got[4].any() and not ref["valid"].any()
    s.slots = keep
    # an empty last frame
    e = orb.Frame(16)
    e.upload(np.zeros(0, orb.KP_DTYPE), np.zeros((0, 32), np.uint8), BOUNDS)
    got = s.F.SearchLastFrame(e, s.mp, np.zeros(0, np.int32), s.cp, s.lp, ps.MB, False, 7, s.sf,
                              np.zeros(len(s.F.kps), np.uint8))
    assert got[0] == 0 and (got[1] == -1).all() and got[3] == 0 and len(got[4]) == 0
    s.compare(7)
    # the call profile hook covers this entry point
    lib, us = orb.load_library(), (C.c_float * 4)()
    assert lib.vsg_debug_call_profile(us) == 0
    fill, launch, sync, total = list(us)
    assert total >= sync > 0 and total < 1e6, list(us)


def test_two_threads_two_frames_one_store(ex):
    scenes = [Scene(ex, 7, False), Scene(ex, 8, True, 2 * ps.MB)]
    # one store holds both scenes' points: the second scene's slots sit behind the first's
    n0 = len(scenes[0].store_slots)
    fields = {k: np.concatenate([s.fields[k] for s in scenes]) for k in ps.FIELDS}
    mp = ps.store_of(fields, np.arange(len(fields["desc"]), dtype=np.int32))
    scenes[1].slots = np.where(scenes[1].slots >= 0, scenes[1].slots + n0, -1).astype(np.int32)
    scenes[1].by_slot = {k: np.concatenate([scenes[0].fields[k], scenes[1].by_slot[k]]) for k in ps.FIELDS}
    for s in scenes:
        s.mp = mp
    want = [s.compare(15)[1] for s in scenes]
    calls, got, errs = 6, [[], []], []
    gate = threading.Barrier(2)

    def run(i):
        try:
            s = scenes[i]
            blocked = np.zeros(len(s.F.kps), np.uint8)
            s.search(15, False, True, blocked)  # the thread's stream and arenas exist from here on
            for _ in range(calls):
                gate.wait(timeout=60)  # both threads enter the call together, every round
                got[i].append(s.search(15, False, True, blocked))
            orb.load_library().vsg_thread_release()
        except Exception as e:  # noqa: BLE001
            gate.abort()
            errs.append(e)
    ts = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errs, errs
    for gs, w in zip(got, want):
        assert len(gs) == calls
        for g in gs:
            assert g[0] == w[0] and g[3] == w[3] and all(np.array_equal(a, b) for a, b in zip(g[1:3], w[1:3]))
            assert all(a.tobytes() == b.tobytes() for a, b in zip(g[4:], w[4:]))


def test_every_error_returns_its_code_and_leaves_the_thread_usable(ex):
    """The "devices that differ" error needs two GPUs: on a one-GPU machine that case is NOT exercised."""
    s = Scene(ex, 9, True)
    lib = orb.load_library()
    n = len(s.F.kps)
    sf = np.ascontiguousarray(s.sf, np.float32)
    _f, _u8, _i32 = C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_int32)

    def raw(cur=s.F.handle, last=s.L.handle, mp=s.mp.handle, slots=s.slots, cp=s.cp, lp=s.lp, nlevels=8, tb=True, tm=True,
            scale=True, direction=None):
        sl = np.ascontiguousarray(slots, np.int32) if slots is not None else None
        b, m = np.zeros(n, np.uint8), np.full(n, -1, np.int32)
        return lib.vsg_frame_search_last_frame(
            cur, last, mp, sl.ctypes.data_as(_i32) if sl is not None else None, C.byref(cp) if cp is not None else None,
            C.byref(lp) if lp is not None else None, ps.MB, 0, 7.0, sf.ctypes.data_as(_f) if scale else None, nlevels, 1,
            b.ctypes.data_as(_u8) if tb else None, m.ctypes.data_as(_i32) if tm else None,
            C.byref(direction) if direction is not None else None, None, None, None, None)

    def after(code, rc):
        assert rc == code, (rc, code)
        s.compare(7)  # a correct call follows on the same thread and matches the reference

    s.compare(7)
    for kw in (dict(cur=None), dict(last=None), dict(mp=None), dict(cp=None), dict(lp=None), dict(tb=False),
               dict(tm=False), dict(scale=False), dict(slots=None)):
        after(-6, raw(**kw))
    after(-6, raw(nlevels=0))
    after(-6, raw(nlevels=17))
    after(-6, raw(nlevels=7))  # pose->n_levels (8) > nlevels
    bad = s.slots.copy()
    bad[np.flatnonzero(bad >= 0)[-1]] = s.mp.capacity
    after(-6, raw(slots=bad))
    d = C.c_int(77)  # an invalid call writes no output; a valid one writes the direction
    after(-6, raw(slots=bad, direction=d))
    assert d.value == 77
    assert raw(direction=d) >= 0 and d.value in (0, 1, 2)
    # a feature that carries a slot and whose octave lies outside [0, nlevels): the existing call refuses this too
    p4 = dict(s.pose, n_levels=4)
    assert (s.lk["octave"][s.slots >= 0] >= 4).any()
    after(-6, raw(cp=orb.FramePose.make(**p4), nlevels=4))
    # ... and the same octaves on features WITHOUT a slot are fine
    low = np.where(s.lk["octave"] >= 4, -1, s.slots).astype(np.int32)
    assert raw(cp=orb.FramePose.make(**p4), nlevels=4, slots=low) >= 0
    # Nleft != -1 on either frame
    half = len(s.lk) // 2
    stereo = orb.Frame(len(s.lk) + 1)
    stereo.upload(s.lk, np.zeros((len(s.lk), 32), np.uint8), BOUNDS, nleft=half)
    after(-3, raw(last=stereo.handle))
    after(-3, raw(cur=stereo.handle))
    if lib.vsg_device_count() > 1:  # devices that differ
        other = orb.MapPoints(16, device=1)
        after(-6, raw(mp=other.handle))
    with pytest.raises(orb.VsgError) as e:
        s.F.SearchLastFrame(s.L, s.mp, bad, s.cp, s.lp, ps.MB, False, 7, s.sf, np.zeros(n, np.uint8))
    assert e.value.code == -6
    with pytest.raises(ValueError):
        s.F.SearchLastFrame(s.L, s.mp, s.slots[:-1], s.cp, s.lp, ps.MB, False, 7, s.sf, np.zeros(n, np.uint8))
    s.compare(7)
