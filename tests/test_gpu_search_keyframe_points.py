"""GPU tests of SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) on resident map points
(vsg_frame_search_keyframe_points) against the EXISTING vsg_frame_search_by_projection_kf (oracle-checked by
tests/test_gpu_frame.py) fed with tests/projection_reference.py's u, v, radius, predicted_level: nmatches, train_match
(mapped back through the index map) and occupied identical; projected, u, v, predicted_level bit-equal to the
restatement.  Scenes as in tests/test_gpu_search_last_frame.py."""
import ctypes as C

import numpy as np
import pytest

import projection_reference as pr
import projection_scenes as ps
from test_gpu_search_last_frame import BOUNDS, ex, make_frame  # noqa: F401  (ex: the module's extractor fixture)
from visual_sgraphs_amd import orb

pytestmark = pytest.mark.gpu


class Scene:
    def __init__(self, ex, seed, rgbd=False, mirror=False, capacity_factor=None, n_other=300):
        self.F, desc, ur = make_frame(ex, seed, rgbd)
        self.pose = ps.current_pose(seed)
        self.fields, src = ps.map_points(self.F.kps, desc, ur, self.pose, 100 + seed, mirror=mirror, n_other=n_other)
        rng = np.random.default_rng(400 + seed)
        n = len(src)
        self.cap = int(capacity_factor * n) + 5 if capacity_factor else n
        # its own generator: the placement in the store does not change the observer's angles
        place = np.random.default_rng(7777 + seed)
        self.slots = (place.permutation(self.cap)[:n] if capacity_factor else np.arange(n)).astype(np.int32)
        self.mp = ps.store_of(self.fields, self.slots, self.cap)
        self.kf_angle = ps.observer_angles(self.F.kps, np.maximum(src, 0), rng)  # pKF->mvKeysUn[i].angle
        self.sf = ex.GetScaleFactors()
        self.cp = orb.FramePose.make(**self.pose)

    def compare(self, th, orb_dist, skip=None, occupied=None, check=True, kf_angle=True, min_match=0.10):
        f = self.fields
        occupied = np.zeros(len(self.F.kps), np.uint8) if occupied is None else occupied
        ref = pr.project_kf_points(self.pose, BOUNDS, f["world_pos"], f["min_dist"], f["max_dist"], skip)
        a = pr.keyframe_fields(ref, np.arange(len(self.slots)), f["desc"], self.kf_angle, th, self.sf)
        want = self.F.SearchByProjection_KF(a["desc"], a["u"], a["v"], a["radius"], a["predicted_level"], a["kf_angle"],
                                            orb_dist, check, occupied)
        want = (want[0], pr.map_back(want[1], a["index"]), want[2])
        n_proj, n_q = int(ref["valid"].sum()), int(len(self.slots) - (0 if skip is None else (skip != 0).sum()))
        print(f"kf n={len(self.slots)} queried {n_q} projected {n_proj} nmatches {want[0]} th {th} ORBdist {orb_dist}")
        if min_match is not None:  # conditions on the fixture and the existing path, not on the code under test
            assert n_proj >= 0.5 * n_q, (n_proj, n_q)
            assert want[0] >= min_match * n_proj, (want[0], n_proj)
        got = self.F.SearchKeyFramePoints(self.mp, self.slots, self.cp, th, orb_dist, self.sf, occupied,
                                          self.kf_angle if kf_angle else None, skip, check)
        assert got[0] == want[0]
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
        assert np.array_equal(got[3], ref["valid"])
        for x, k in ((got[4], "u"), (got[5], "v"), (got[6], "level")):
            assert x.dtype == ref[k].dtype and x.tobytes() == ref[k].tobytes(), k
        return want, got, ref


@pytest.mark.parametrize("rgbd", [False, True], ids=["gray", "rgbd"])
@pytest.mark.parametrize("th,orb_dist", [(10, 100), (3, 64)])  # Tracking.cc:3805, :3819
def test_equal_to_search_by_projection_kf(ex, rgbd, th, orb_dist):
    s = Scene(ex, 3, rgbd)
    base, _, ref = s.compare(th, orb_dist)
    v = ref["valid"] != 0
    assert len(set(ref["level"][v].tolist())) >= 6 and not v.all()
    rng = np.random.default_rng(th)
    # skip on a fifth of the points: none of them is matched
    skip = (rng.random(len(s.slots)) < 0.2).astype(np.uint8)
    _, got, _ = s.compare(th, orb_dist, skip=skip)
    assert not np.isin(got[1], np.flatnonzero(skip)).any() and not got[3][skip != 0].any()
    # occupied pre-set on a tenth of the features: none of them is taken
    occ = (rng.random(len(s.F.kps)) < 0.1).astype(np.uint8)
    _, got, _ = s.compare(th, orb_dist, occupied=occ)
    assert (got[1][occ != 0] == -1).all()
    # the rotation filter off, with and without the angles
    off, _, _ = s.compare(th, orb_dist, check=False)
    off2, _, _ = s.compare(th, orb_dist, check=False, kf_angle=False)
    assert off[0] >= base[0] and off2[0] == off[0]


def test_points_behind_the_camera_are_not_rejected_by_sign(ex):
    """The reference has no invzc test here (ORBmatcher.cc:1905-1912): a point behind the camera that projects into the
    image is searched like any other.  The restatement keeps them and the results still agree."""
    s = Scene(ex, 4, mirror=True)
    want, got, ref = s.compare(10, 100)
    v = ref["valid"] != 0
    assert (ref["z"][v] < 0).mean() > 0.8 and want[0] > 0.1 * v.sum()
    front = Scene(ex, 4)
    w2, _, _ = front.compare(10, 100)
    assert w2[0] > 0


def test_band_ends(ex):
    """dist3D == 0.8f * mfMinDistance and == 1.2f * mfMaxDistance are inside; a ten-thousandth further is outside."""
    s = Scene(ex, 5, n_other=0)
    f = s.fields
    PO = [(f["world_pos"][:, i] - s.pose["Ow"][i]).astype(np.float32) for i in range(3)]
    dist = np.sqrt(pr._dot3(PO[0], PO[1], PO[2], PO[0], PO[1], PO[2])).astype(np.float32)
    k = len(dist) // 4

    def smallest_member(factor):  # the smallest member m with factor * m >= dist
        m = (dist / np.float32(factor)).astype(np.float32)
        for _ in range(4):
            low = (np.float32(factor) * m).astype(np.float32) < dist
            m = np.where(low, np.nextafter(m, np.float32(np.inf)), m).astype(np.float32)
        for _ in range(4):
            down = np.nextafter(m, np.float32(0))
            m = np.where((np.float32(factor) * down).astype(np.float32) >= dist, down, m).astype(np.float32)
        return m, (np.float32(factor) * m).astype(np.float32) == dist
    mn, on_min = smallest_member(0.8)
    mx, on_max = smallest_member(1.2)
    f["min_dist"][:k] = np.where(on_min[:k], mn[:k], f["min_dist"][:k])                      # dist == 0.8f * mfMinDistance
    f["min_dist"][k:2 * k] = mn[k:2 * k] * np.float32(1.0001)                                # dist below the band
    f["max_dist"][2 * k:3 * k] = np.where(on_max[2 * k:3 * k], mx[2 * k:3 * k], f["max_dist"][2 * k:3 * k])  # == 1.2f * mfMax
    f["max_dist"][3 * k:] = mx[3 * k:] * np.float32(0.9999)                                  # dist above the band
    assert on_min[:k].sum() > 20 and on_max[2 * k:3 * k].sum() > 20
    s.mp.update(s.slots, min_dist=f["min_dist"], max_dist=f["max_dist"])
    _, _, ref = s.compare(10, 100, min_match=None)
    assert ref["valid"][:k][on_min[:k]].all() and not ref["valid"][k:2 * k].any()
    assert ref["valid"][2 * k:3 * k][on_max[2 * k:3 * k]].all() and not ref["valid"][3 * k:].any()


def test_permuted_store_empty_list_and_errors(ex):
    """The "devices that differ" error needs two GPUs and is NOT exercised here: the suite runs on one."""
    s = Scene(ex, 6, True, capacity_factor=2.0)
    base = Scene(ex, 6, True)
    w0, _, _ = base.compare(10, 100)
    w1, _, _ = s.compare(10, 100)
    assert w0[0] == w1[0] and np.array_equal(w0[1], w1[1])  # train_match holds QUERY indices either way
    n = len(s.F.kps)
    occ = np.zeros(n, np.uint8)
    got = s.F.SearchKeyFramePoints(s.mp, np.zeros(0, np.int32), s.cp, 10, 100, s.sf, occ)
    assert got[0] == 0 and (got[1] == -1).all() and len(got[3]) == 0
    lib = orb.load_library()
    sf = np.ascontiguousarray(s.sf, np.float32)
    _f, _u8, _i32 = C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_int32)

    def raw(cur=s.F.handle, mp=s.mp.handle, slots=s.slots, cp=s.cp, nlevels=8, angle=True, check=1, oc=True, tm=True,
            scale=True, n=None, null_slots=False):
        sl = np.ascontiguousarray(slots, np.int32)
        b, m = np.zeros(len(s.F.kps), np.uint8), np.full(len(s.F.kps), -1, np.int32)
        return lib.vsg_frame_search_keyframe_points(
            cur, mp, len(sl) if n is None else n, None if null_slots else sl.ctypes.data_as(_i32), None,
            C.byref(cp) if cp is not None else None,
            10.0, 100, sf.ctypes.data_as(_f) if scale else None, nlevels, check,
            s.kf_angle.ctypes.data_as(_f) if angle else None, b.ctypes.data_as(_u8) if oc else None,
            m.ctypes.data_as(_i32) if tm else None, None, None, None, None)

    def after(code, rc):
        assert rc == code, (rc, code)
        s.compare(10, 100)  # a correct call follows on the same thread and matches the reference

    for kw in (dict(cur=None), dict(mp=None), dict(cp=None), dict(oc=False), dict(tm=False), dict(scale=False),
               dict(angle=False), dict(null_slots=True), dict(n=-1), dict(nlevels=0), dict(nlevels=17),
               dict(nlevels=7)):
        after(-6, raw(**kw))
    assert raw(angle=False, check=0) == s.compare(10, 100, check=False)[1][0]
    for bad_slot in (-1, s.cap):
        bad = s.slots.copy()
        bad[-1] = bad_slot
        after(-6, raw(slots=bad))
    stereo = orb.Frame(len(s.F.kps) + 1)
    stereo.upload(s.F.kps, np.zeros((len(s.F.kps), 32), np.uint8), BOUNDS, nleft=len(s.F.kps) // 2)
    after(-3, raw(cur=stereo.handle))
    with pytest.raises(ValueError):
        s.F.SearchKeyFramePoints(s.mp, s.slots, s.cp, 10, 100, s.sf, occ, skip=np.zeros(3, np.uint8))
