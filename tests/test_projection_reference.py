"""CPU tests of the projection geometry of the motion-model and relocalisation searches: tests/projection_reference.py
(written from ORBmatcher.cc:1677-1709, :1744, :1904-1928) against visual_sgraphs_amd/csrc/vsg_project.h compiled for the
host by tests/_projectcore, bit for bit, and both against cases worked out by hand."""
import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import frustum_reference as fr
import projection_reference as pr
from visual_sgraphs_amd import orb

F32 = np.float32
PC_DIR = Path(__file__).resolve().parent / "_projectcore"
BOUNDS = (0.0, 0.0, 640.0, 480.0)
_f32p, _u8p, _i32p = (C.POINTER(t) for t in (C.c_float, C.c_uint8, C.c_int32))
_pose = C.POINTER(orb.FramePose)


@pytest.fixture(scope="module")
def pc():
    asan = bool(os.environ.get("VSG_PROJECTCORE_ASAN"))  # tests/test_sanitizers_projection.py: the ASan + UBSan build
    subprocess.check_call(["make", "-C", str(PC_DIR)] + (["asan"] if asan else []), stdout=subprocess.DEVNULL)
    L = C.CDLL(str(PC_DIR / ("libvsg_projectcore_asan.so" if asan else "libvsg_projectcore.so")))
    L.pc_project_last.restype = None
    L.pc_project_last.argtypes = [_pose, _f32p, C.c_int, _f32p, _u8p, _u8p, _f32p, _f32p, _f32p]
    L.pc_project_kf.restype = None
    L.pc_project_kf.argtypes = [_pose, _f32p, C.c_int, _f32p, _f32p, _f32p, _u8p, _u8p, _f32p, _f32p, _i32p]
    L.pc_motion_direction.argtypes = [_pose, _pose, C.c_float, C.c_int]
    return L


def _c(a, dtype):
    return np.ascontiguousarray(a, dtype)


def host_last(pc, pose, bounds, P, active=None):
    P = _c(P, F32).reshape(-1, 3)
    n = len(P)
    out = dict(valid=np.zeros(n, np.uint8), u=np.zeros(n, F32), v=np.zeros(n, F32), ur=np.zeros(n, F32))
    act = _c(active, np.uint8) if active is not None else None
    pc.pc_project_last(C.byref(orb.FramePose.make(**pose)), _c(bounds, F32).ctypes.data_as(_f32p), n,
                       P.ctypes.data_as(_f32p), act.ctypes.data_as(_u8p) if act is not None else None,
                       out["valid"].ctypes.data_as(_u8p), out["u"].ctypes.data_as(_f32p), out["v"].ctypes.data_as(_f32p),
                       out["ur"].ctypes.data_as(_f32p))
    return out


def host_kf(pc, pose, bounds, P, mf_min, mf_max, skip=None):
    P = _c(P, F32).reshape(-1, 3)
    n = len(P)
    out = dict(valid=np.zeros(n, np.uint8), u=np.zeros(n, F32), v=np.zeros(n, F32), level=np.zeros(n, np.int32))
    sk = _c(skip, np.uint8) if skip is not None else None
    mn, mx = _c(mf_min, F32), _c(mf_max, F32)
    pc.pc_project_kf(C.byref(orb.FramePose.make(**pose)), _c(bounds, F32).ctypes.data_as(_f32p), n,
                     P.ctypes.data_as(_f32p), mn.ctypes.data_as(_f32p), mx.ctypes.data_as(_f32p),
                     sk.ctypes.data_as(_u8p) if sk is not None else None, out["valid"].ctypes.data_as(_u8p),
                     out["u"].ctypes.data_as(_f32p), out["v"].ctypes.data_as(_f32p), out["level"].ctypes.data_as(_i32p))
    return out


def assert_bit_equal(got, ref, keys):
    """Every point, every field, as bit patterns (so NaN equals NaN); no tolerance."""
    for k in keys:
        a, b = np.asarray(got[k]), np.asarray(ref[k])
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), k


def unit_pose(**kw):
    # powers of two: u = 512 X / Z + 320, v = 512 Y / Z + 240 are exact for the points below
    return fr.make_pose(np.eye(3), np.zeros(3), 512.0, 512.0, 320.0, 240.0, 40.0, **kw)


@pytest.mark.parametrize("camera", sorted(fr.CAMERAS))
def test_host_projection_is_bit_equal_to_the_reference(pc, camera):
    for seed in range(8):
        pose, bounds, f = fr.scenario(seed, camera)
        rng = np.random.default_rng(seed)
        active = (rng.random(len(f["world_pos"])) < 0.8).astype(np.uint8)
        ref = pr.project_last_points(pose, bounds, f["world_pos"], active)
        # the scenario exercises every exit: inactive, behind, outside, projected
        assert 0.1 < ref["valid"].mean() < 0.7 and np.isfinite(ref["ur"]).all()
        assert_bit_equal(host_last(pc, pose, bounds, f["world_pos"], active), ref, ("valid", "u", "v", "ur"))
        skip = (rng.random(len(active)) < 0.2).astype(np.uint8)
        ref = pr.project_kf_points(pose, bounds, f["world_pos"], f["min_dist"], f["max_dist"], skip)
        v = ref["valid"] != 0
        assert 0.05 < v.mean() < 0.7 and len(set(ref["level"][v].tolist())) >= 6
        assert (ref["z"][v] < 0).any()  # no sign test: points behind the camera are kept
        assert_bit_equal(host_kf(pc, pose, bounds, f["world_pos"], f["min_dist"], f["max_dist"], skip), ref,
                         ("valid", "u", "v", "level"))


def test_last_frame_edges(pc):
    """z == 0, z < 0, exactly on each bound and just outside, NaN coordinates."""
    nan = np.nan
    P = np.array([(0, 0, 4),                                                       # the optical axis
                  (-2.5, 0, 4), (2.5, 0, 4), (0, -1.875, 4), (0, 1.875, 4),        # u = 0, 640; v = 0, 480: inside
                  (-2.5025, 0, 4), (2.5025, 0, 4), (0, -1.877, 4), (0, 1.877, 4),  # a thousandth further: outside
                  (0, 0, -4),                                                      # invzc < 0
                  (1, 0, 0),                                                       # z == +0: invzc = +inf, u = +inf: outside
                  (0, 0, 0),                                                       # 0 / 0: NaN passes every comparison
                  (nan, 0, 4), (0, nan, 4), (0, 0, nan)], F32)
    ref = pr.project_last_points(unit_pose(), BOUNDS, P)
    assert ref["valid"].tolist() == [1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1]
    assert (ref["u"][0], ref["v"][0], ref["ur"][0]) == (F32(320), F32(240), F32(310))  # 320 - 40 * (1 / 4)
    assert ref["u"][1:5].tolist() == [0, 640, 320, 320] and ref["v"][1:5].tolist() == [240, 240, 0, 480]
    assert np.isnan(ref["u"][11]) and np.isnan(ref["v"][11]) and np.isnan(ref["ur"][11])
    # 0 * NaN = NaN: one NaN coordinate reaches every row of Rcw * P
    assert all(np.isnan(ref[k][12:15]).all() for k in ("u", "v", "ur"))
    assert_bit_equal(host_last(pc, unit_pose(), BOUNDS, P), ref, ("valid", "u", "v", "ur"))
    # inactive features are never projected
    act = np.zeros(len(P), np.uint8)
    assert not pr.project_last_points(unit_pose(), BOUNDS, P, act)["valid"].any()
    assert not host_last(pc, unit_pose(), BOUNDS, P, act)["valid"].any()


def test_keyframe_edges(pc):
    """No sign test, the bounds, the band's two ends (closed), PredictScale on the member, NaN."""
    z6 = F32(1.2) * F32(5)
    cases = [((0, 0, 4), 0.5, 6.0, 1, 3),        # log(1.5) / log(1.2) = 2.22 -> level 3
             ((0, 0, 4), 0.5, 4.0, 1, 0),        # the ratio uses the MEMBER mfMaxDistance: log 1 = 0 -> level 0
             ((0, 0, 4), 0.01, 400.0, 1, 7),     # clamped to n_levels - 1
             ((0, 0, -4), 0.5, 6.0, 1, 3),       # BEHIND the camera: u = 320, v = 240 again, and it is kept
             ((2.5, 0, -4), 0.5, 6.0, 1, None),  # behind and mirrored: u = 0
             ((-2.5, 0, 4), 0.5, 6.0, 1, None), ((2.5025, 0, 4), 0.5, 6.0, 0, None),
             ((0, 1.875, 4), 0.5, 6.0, 1, None), ((0, 1.877, 4), 0.5, 6.0, 0, None),
             ((0, 0, 4), 5.0, 20.0, 1, None),                                # dist == 0.8f * mfMinDistance
             ((0, 0, 4), np.nextafter(F32(5), F32(6)), 20.0, 0, None),       # just below the band
             ((0, 0, z6), 0.5, 5.0, 1, 0),                                   # dist == 1.2f * mfMaxDistance; ratio < 1 -> 0
             ((0, 0, np.nextafter(z6, F32(7))), 0.5, 5.0, 0, None),          # just above
             ((1, 0, 0), 0.0, 6.0, 0, None),                                 # z == 0: u = inf
             ((0, 0, 0), 0.0, 6.0, 1, 0),                                    # NaN u, v pass; dist 0 -> INT_MIN -> 0
             ((np.nan, 0, 4), 0.5, 6.0, 1, 0)]                               # NaN dist passes the band; NaN level -> 0
    assert F32(0.8) * F32(5) == F32(4)
    P = np.array([c[0] for c in cases], F32)
    mn, mx = np.array([c[1] for c in cases], F32), np.array([c[2] for c in cases], F32)
    ref = pr.project_kf_points(unit_pose(), BOUNDS, P, mn, mx)
    assert ref["valid"].tolist() == [c[3] for c in cases]
    for i, c in enumerate(cases):
        if c[4] is not None:
            assert ref["level"][i] == c[4], i
    assert (ref["u"][3], ref["v"][3]) == (F32(320), F32(240)) and ref["u"][4] == F32(0)
    assert_bit_equal(host_kf(pc, unit_pose(), BOUNDS, P, mn, mx), ref, ("valid", "u", "v", "level"))
    skip = np.ones(len(P), np.uint8)
    assert not pr.project_kf_points(unit_pose(), BOUNDS, P, mn, mx, skip)["valid"].any()
    assert not host_kf(pc, unit_pose(), BOUNDS, P, mn, mx, skip)["valid"].any()


def test_motion_direction_at_the_baseline(pc):
    """tlc_z == +-mb is neither (strict '>'); one ulp further is forward / backward; bMono switches both off."""
    mb = F32(0.125)
    last = unit_pose()
    up, dn = np.nextafter(mb, F32(1)), np.nextafter(mb, F32(0))
    want = {mb: 0, up: 1, dn: 0, -mb: 0, -up: 2, -dn: 0, F32(0): 0, F32(2) * mb: 1, F32(-2) * mb: 2}
    for z, d in want.items():
        cur = unit_pose(Ow=(0.5, -0.25, z))  # Ow is what the caller passes: tlc_z = Ow_z exactly for an identity last pose
        for mono in (0, 1):
            exp = 0 if mono else d
            assert pr.motion_direction(cur, last, mb, mono) == exp, (z, mono)
            assert pc.pc_motion_direction(C.byref(orb.FramePose.make(**cur)), C.byref(orb.FramePose.make(**last)), mb,
                                          mono) == exp, (z, mono)
    # general poses: the restatement and the header agree, and both directions occur
    seen = set()
    for seed in range(40):
        a, _, _ = fr.scenario(seed, "euroc", n=1)
        b, _, _ = fr.scenario(seed + 100, "euroc", n=1)
        d = pr.motion_direction(a, b, 0.11, 0)
        assert d == pc.pc_motion_direction(C.byref(orb.FramePose.make(**a)), C.byref(orb.FramePose.make(**b)), 0.11, 0)
        seen.add(d)
    assert seen == {0, 1, 2}


def test_compacted_fields_and_index_map():
    pose, bounds, f = fr.scenario(1, "tum1", n=300)
    rng = np.random.default_rng(1)
    slots = rng.permutation(300).astype(np.int32)
    slots[::7] = -1
    kps = np.zeros(300, orb.KP_DTYPE)
    kps["octave"], kps["angle"] = rng.integers(0, 8, 300), rng.uniform(0, 360, 300)
    P = f["world_pos"][np.maximum(slots, 0)]
    ref = pr.project_last_points(pose, bounds, P, slots >= 0)
    a = pr.last_frame_fields(ref, slots, kps, f["desc"], f["observed"])
    assert len(a["index"]) == ref["valid"].sum() and (np.diff(a["index"]) > 0).all() and (slots[a["index"]] >= 0).all()
    assert np.array_equal(a["desc"], f["desc"][slots[a["index"]]]) and np.array_equal(a["last_octave"], kps["octave"][a["index"]])
    tm = np.array([-1, 0, len(a["index"]) - 1])
    assert pr.map_back(tm, a["index"]).tolist() == [-1, a["index"][0], a["index"][-1]]
    sf = (F32(1.2) ** np.arange(8, dtype=F32)).astype(F32)
    rk = pr.project_kf_points(pose, bounds, f["world_pos"], f["min_dist"], f["max_dist"])
    b = pr.keyframe_fields(rk, np.arange(300), f["desc"], None, 10, sf)
    assert b["radius"].dtype == F32 and np.array_equal(b["radius"], (F32(10) * sf[b["predicted_level"]]).astype(F32))
