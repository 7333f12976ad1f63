"""GPU tests of Fuse x2 and SearchByProjection(pKF, Scw, ...) on resident map points (vsg_frame_fuse_points,
vsg_frame_fuse_points_sim3, vsg_frame_search_sim3_points) against the EXISTING vsg_frame_fuse / vsg_frame_fuse_sim3 /
vsg_frame_search_by_projection_sim3 (oracle-checked by tests/test_gpu_frame.py) fed with
tests/keyframe_projection_reference.py's u, v, ur, radius, predicted_level: the return value, best_idx, best_dist and
matched (mapped back through the index map) identical; projected, u, v, ur, predicted_level byte-equal to the restatement.
The target KeyFrame is a real extracted frame (gray and RGB-D, so both branches of the chi-square gate are live); the map
points are its keypoints un-projected through its pose (tests/keyframe_scenes.py).  The Sim3 routines take the pose their
caller decomposed Scw into, so one pose serves all three."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import keyframe_projection_reference as kr
import keyframe_scenes as ks
import projection_scenes as ps
from test_abi_projection import _blob, _cam, _load
from test_gpu_search_last_frame import BOUNDS, ex, make_frame  # noqa: F401  (ex: the module's extractor fixture)
from visual_sgraphs_amd import orb

pytestmark = pytest.mark.gpu
TH_LOW, INT_MAX = 50, 0x7FFFFFFF
SET = 1 << 20  # a vpMatched entry that is set on entry
ADAPTOR = Path(__file__).resolve().parent / "_adaptor_keyframe"


class Scene:
    def __init__(self, ex, seed, rgbd=False, mirror=False, capacity_factor=None, n_other=300, bounds=BOUNDS):
        self.F, desc, self.ur = make_frame(ex, seed, rgbd)
        if bounds != BOUNDS:  # the same features in a KeyFrame whose image bounds have fractions
            kps = self.F.kps.copy()
            self.F = orb.Frame(len(kps) + 1)
            self.F.upload(kps, desc, bounds, u_right=self.ur)
        self.bounds, self.kf_desc = bounds, desc
        self.pose = ps.current_pose(seed)
        self.fields, self.src = ks.keyframe_map(self.F.kps, desc, self.ur, self.pose, 100 + seed, n_other, mirror=mirror)
        n = len(self.src)
        self.cap = int(capacity_factor * n) + 5 if capacity_factor else n
        place = np.random.default_rng(7777 + seed)
        self.slots = (place.permutation(self.cap)[:n] if capacity_factor else np.arange(n)).astype(np.int32)
        self.mp = ps.store_of(self.fields, self.slots, self.cap)
        self.sf, self.inv2 = ex.GetScaleFactors(), ex.GetInverseScaleSigmaSquares()
        self.cp = orb.FramePose.make(**self.pose)

    def reference(self, th, q, skip):
        """The restatement for the queries q (indices of points) and the compacted arrays of the existing entries."""
        f = self.fields
        ref = kr.project_keyframe_points(self.pose, self.bounds, f["world_pos"][q], f["normal"][q], f["min_dist"][q],
                                         f["max_dist"][q], skip)
        return ref, kr.fuse_fields(ref, np.arange(len(q)), f["desc"][q], th, self.sf)

    def compare(self, entry, th, q=None, skip=None, ratio=1.0, matched=None, conditions=False):
        """entry: "fuse", "fuse_sim3" or "search".  conditions: those on the fixture and the existing path, asked before
        the code under test runs."""
        q = np.arange(len(self.slots)) if q is None else np.asarray(q)
        n = len(q)
        ref, a = self.reference(th, q, skip)
        idx = a["index"]
        if entry == "search":
            matched = np.full(len(self.F.kps), -1, np.int32) if matched is None else matched
            nm, m = self.F.SearchByProjection_Sim3(a["desc"], a["u"], a["v"], a["radius"], a["predicted_level"], ratio, matched)
            new = m != matched
            m = m.copy()
            m[new] = idx[m[new]]
            want = (nm, m)
            print(f"search n={n} projected {len(idx)} nmatches {nm} th {th} ratio {ratio}")
            if conditions:
                kr.check_scene(ref)
                assert nm >= 1
            got = self.F.SearchSim3Points(self.mp, self.slots[q], self.cp, th, ratio, self.sf, matched, skip)
            assert got[0] == want[0] and np.array_equal(got[1], want[1])
            proj = got[2:]
        else:
            sim3 = entry == "fuse_sim3"
            if sim3:
                w = self.F.Fuse_Sim3(a["desc"], a["u"], a["v"], a["radius"], a["predicted_level"])
            else:
                w = self.F.Fuse(a["desc"], a["u"], a["v"], a["ur"], a["radius"], a["predicted_level"], self.inv2)
            want = (w[0], kr.spread(idx, n, w[1], -1), kr.spread(idx, n, w[2], INT_MAX if sim3 else 256))
            print(f"{entry} n={n} projected {len(idx)} fused {w[0]} beyond TH_LOW {int(((w[1] >= 0) & (w[2] > TH_LOW)).sum())} th {th}")
            if conditions:
                kr.check_scene(ref)
                assert w[0] >= 1 and ((w[1] >= 0) & (w[2] > TH_LOW)).any()
            if sim3:
                got = self.F.FusePoints_Sim3(self.mp, self.slots[q], self.cp, th, self.sf, skip)
                proj = got[3:]
            else:
                got = self.F.FusePoints(self.mp, self.slots[q], self.cp, th, self.sf, self.inv2, skip)
                proj = got[3:6] + got[7:]
                assert got[6].dtype == ref["ur"].dtype and got[6].tobytes() == ref["ur"].tobytes()
            assert got[0] == want[0]
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
        assert np.array_equal(proj[0], ref["valid"])
        for x, k in zip(proj[1:], ("u", "v", "level")):
            assert x.dtype == ref[k].dtype and x.tobytes() == ref[k].tobytes(), k  # bit patterns
        return want, got, ref


ENTRIES = [("fuse", 3, 1.0), ("fuse_sim3", 4, 1.0), ("search", 8, 1.5), ("search", 5, 1.0), ("search", 3, 1.5)]
IDS = ["fuse-th3", "fuse_sim3-th4", "search-th8-r1.5", "search-th5-r1.0", "search-th3-r1.5"]


@pytest.fixture(scope="module")
def scenes(ex):
    return {rgbd: Scene(ex, 3, rgbd) for rgbd in (False, True)}


@pytest.mark.parametrize("rgbd", [False, True], ids=["gray", "rgbd"])
@pytest.mark.parametrize("entry,th,ratio", ENTRIES, ids=IDS)
def test_equal_to_the_existing_entry(scenes, rgbd, entry, th, ratio):
    s = scenes[rgbd]
    if rgbd:  # both branches of the chi-square gate: keypoints with and without mvuRight
        assert (s.ur >= 0).sum() > 100 and (s.ur < 0).sum() > 10
    _, _, ref = s.compare(entry, th, ratio=ratio, conditions=True)
    v = ref["valid"] != 0
    assert len(set(ref["level"][v].tolist())) >= 6 and not v.all()
    rng = np.random.default_rng(th)
    # skip on a fifth of the points: none of them is projected or matched
    skip = (rng.random(len(s.slots)) < 0.2).astype(np.uint8)
    _, got, _ = s.compare(entry, th, skip=skip, ratio=ratio, conditions=True)
    sk = np.flatnonzero(skip)
    if entry == "search":
        assert not got[2][sk].any() and not np.isin(got[1], sk).any()
        # matched pre-set on a tenth of the features: none of those is taken
        pre = np.where(rng.random(len(s.F.kps)) < 0.1, SET, -1).astype(np.int32)
        _, got, _ = s.compare(entry, th, ratio=ratio, matched=pre, conditions=True)
        assert (got[1][pre == SET] == SET).all() and (pre == SET).sum() > 50
    else:
        assert not got[3][sk].any() and (got[1][sk] == -1).all()
        assert (got[2][sk] == (INT_MAX if entry == "fuse_sim3" else 256)).all()


def test_the_chi_square_gate_is_live(scenes):
    """With th 3 the gate (5.99 / 7.8 at the keypoint's level) removes candidates the Sim3 form keeps: the two existing
    entries differ on the same points, and each resident entry follows its own."""
    s = scenes[True]
    a, _, _ = s.compare("fuse", 3)
    b, _, _ = s.compare("fuse_sim3", 3)
    assert not np.array_equal(a[1], b[1])


@pytest.mark.parametrize("entry,th,ratio", ENTRIES[:3], ids=IDS[:3])
def test_kernel_edges(ex, entry, th, ratio):
    """64 lanes per workgroup in the projection kernel, 4 queries per workgroup in the window kernel; a store larger than n
    with permuted slots; a KeyFrame whose bounds truncate (-26.6 -> -26, 671.3 -> 671)."""
    s = Scene(ex, 6, True, capacity_factor=2.0, bounds=ks.FRACTIONAL_BOUNDS)
    s.compare(entry, th, ratio=ratio, conditions=True)
    order = np.random.default_rng(6).permutation(len(s.slots))
    for n in (1, 4, 5, 63, 64, 65):
        s.compare(entry, th, q=order[:n], ratio=ratio)
    # a slot list with repeats: every copy is a query of its own
    q = np.repeat(order[:40], 3)[:101]
    _, _, ref = s.compare(entry, th, q=q, ratio=ratio)
    assert ref["valid"].sum() > 30
    # all points skipped
    _, got, ref = s.compare(entry, th, skip=np.ones(len(s.slots), np.uint8), ratio=ratio)
    assert got[0] == 0 and not ref["valid"].any()


@pytest.mark.parametrize("entry,th,ratio", ENTRIES[:3], ids=IDS[:3])
def test_all_points_behind_the_camera(ex, entry, th, ratio):
    s = Scene(ex, 4, mirror=True, n_other=0)
    _, got, ref = s.compare(entry, th, ratio=ratio)
    assert (ref["why"] == kr.BEHIND).all() and got[0] == 0
    if entry == "search":
        assert (got[1] == -1).all()
    else:
        assert (got[1] == -1).all() and (got[2] == (INT_MAX if entry == "fuse_sim3" else 256)).all()


def test_empty_target_keyframe(scenes):
    s = scenes[False]
    e = orb.Frame(8)
    e.upload(np.zeros(0, orb.KP_DTYPE), np.zeros((0, 32), np.uint8), BOUNDS)
    f = s.fields
    ref = kr.project_keyframe_points(s.pose, BOUNDS, f["world_pos"], f["normal"], f["min_dist"], f["max_dist"])
    got = e.FusePoints(s.mp, s.slots, s.cp, 3, s.sf, s.inv2)
    assert got[0] == 0 and (got[1] == -1).all() and (got[2] == 256).all() and np.array_equal(got[3], ref["valid"])
    assert got[6].tobytes() == ref["ur"].tobytes()
    got = e.FusePoints_Sim3(s.mp, s.slots, s.cp, 4, s.sf)
    assert got[0] == 0 and (got[1] == -1).all() and (got[2] == INT_MAX).all() and np.array_equal(got[3], ref["valid"])
    got = e.SearchSim3Points(s.mp, s.slots, s.cp, 8, 1.5, s.sf, np.zeros(0, np.int32))
    assert got[0] == 0 and len(got[1]) == 0 and np.array_equal(got[2], ref["valid"])
    # and no queries at all
    got = s.F.FusePoints(s.mp, np.zeros(0, np.int32), s.cp, 3, s.sf, s.inv2)
    assert got[0] == 0 and len(got[1]) == 0
    s.compare("fuse", 3)


def test_errors_leave_nothing_running(ex):
    """The "devices that differ" error needs two GPUs and is NOT exercised here: the suite runs on one."""
    s = Scene(ex, 6, True, capacity_factor=2.0)
    none = np.full(len(s.F.kps), -1, np.int32)
    calls = {"fuse": lambda F, sl, sf=s.sf, cp=s.cp: F.FusePoints(s.mp, sl, cp, 3, sf, np.resize(s.inv2, len(sf))),
             "fuse_sim3": lambda F, sl, sf=s.sf, cp=s.cp: F.FusePoints_Sim3(s.mp, sl, cp, 4, sf),
             "search": lambda F, sl, sf=s.sf, cp=s.cp: F.SearchSim3Points(s.mp, sl, cp, 8, 1.5, sf, none)}
    stereo = orb.Frame(len(s.F.kps) + 1)
    stereo.upload(s.F.kps, np.zeros((len(s.F.kps), 32), np.uint8), BOUNDS, nleft=len(s.F.kps) // 2)
    deep = orb.FramePose.make(**dict(s.pose, n_levels=9))
    for entry, call in calls.items():
        th = {"fuse": 3, "fuse_sim3": 4, "search": 8}[entry]
        for bad_slot in (-1, s.cap):  # a negative slot, a slot at capacity
            bad = s.slots.copy()
            bad[len(bad) // 2] = bad_slot
            with pytest.raises(orb.VsgError) as e:
                call(s.F, bad)
            assert e.value.code == -6
            s.compare(entry, th, ratio=1.5)  # a correct call follows on the same thread and agrees
        with pytest.raises(orb.VsgError) as e:  # bRight / mpCamera2
            call(stereo, s.slots)
        assert e.value.code == -3
        for kw in (dict(sf=s.sf[:0]), dict(sf=np.ones(17, np.float32)), dict(cp=deep)):  # nlevels 0, 17; n_levels > nlevels
            with pytest.raises(orb.VsgError) as e:
                call(s.F, s.slots, **kw)
            assert e.value.code == -6
        s.compare(entry, th, ratio=1.5)
    with pytest.raises(ValueError):
        s.F.FusePoints(s.mp, s.slots, s.cp, 3, s.sf, s.inv2, skip=np.zeros(3, np.uint8))


@pytest.mark.parametrize("rgbd", [False, True], ids=["gray", "rgbd"])
def test_cpp_adaptor_agrees_with_the_python_binding(scenes, tmp_path, rgbd):
    """tests/_adaptor_keyframe: the three overloads from plain C++, the map in slots 2 i + 1 of a store twice its size."""
    subprocess.check_call(["make", "-C", str(ADAPTOR)], stdout=subprocess.DEVNULL)
    s = scenes[rgbd]
    f, n = s.fields, len(s.slots)
    rng = np.random.default_rng(31)
    skip = (rng.random(n) < 0.2).astype(np.uint8)
    pre = np.where(rng.random(len(s.F.kps)) < 0.1, SET, -1).astype(np.int32)
    th_fuse, th_loop, th_search, ratio = 3.0, 4.0, 8, 1.5
    src, out = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(b"".join([
        _blob(_cam(s.pose), np.float32), _blob([s.pose["n_levels"], th_search], np.int32),
        _blob(list(BOUNDS) + [th_fuse, th_loop, ratio], np.float32), _blob(s.sf, np.float32), _blob(s.inv2, np.float32),
        _blob(s.F.kps, orb.KP_DTYPE), _blob(s.kf_desc, np.uint8), _blob(s.ur if rgbd else np.zeros(0), np.float32),
        _blob(f["world_pos"], np.float32), _blob(f["normal"], np.float32), _blob(f["min_dist"], np.float32),
        _blob(f["max_dist"], np.float32), _blob(f["desc"], np.uint8), _blob(skip, np.uint8), _blob(pre, np.int32)]))
    r = subprocess.run([str(ADAPTOR / "keyframe_check"), str(src), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    buf, pos, got = out.read_bytes(), 0, {}
    for name, dt in (("head", np.int32), ("bi", np.int32), ("bd", np.int32), ("proj", np.uint8), ("u", np.float32),
                     ("v", np.float32), ("ur", np.float32), ("level", np.int32), ("bi3", np.int32), ("bd3", np.int32),
                     ("proj3", np.uint8), ("level3", np.int32), ("matched", np.int32), ("sproj", np.uint8),
                     ("su", np.float32), ("sv", np.float32), ("slevel", np.int32)):
        got[name], pos = _load(buf, pos, dt)
    assert pos == len(buf) and got["head"][3] == len(s.F.kps)
    py = s.F.FusePoints(s.mp, s.slots, s.cp, th_fuse, s.sf, s.inv2, skip)
    assert py[0] == got["head"][0] >= 1
    for a, k in zip(py[1:], ("bi", "bd", "proj", "u", "v", "ur", "level")):
        assert a.tobytes() == got[k].tobytes(), k
    py = s.F.FusePoints_Sim3(s.mp, s.slots, s.cp, th_loop, s.sf, skip)
    assert py[0] == got["head"][1] >= 1
    for a, k in zip((py[1], py[2], py[3], py[6]), ("bi3", "bd3", "proj3", "level3")):
        assert a.tobytes() == got[k].tobytes(), k
    py = s.F.SearchSim3Points(s.mp, s.slots, s.cp, th_search, ratio, s.sf, pre, skip)
    assert py[0] == got["head"][2] >= 1
    for a, k in zip(py[1:], ("matched", "sproj", "su", "sv", "slevel")):
        assert a.tobytes() == got[k].tobytes(), k
