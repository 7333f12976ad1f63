"""Which per-point output blocks exist in a call on resident map points (vsg_mappoints.hip: PointOut / PointStage): every
entry point called straight through ctypes with all of its optional outputs, with none of them, and with every second one
NULL.  The return value, the required outputs and every optional output that was given must be identical across the
three calls; the two entries that take a NULL slot list must give with it what they give with slots 0 .. n-1.  An entry is
only compared with itself here; that its values are right is tests/test_gpu_frustum.py's, test_gpu_search_*.py's and
test_gpu_keyframe_points.py's business.

Sizes: 1, 4, 5 (a second 4-query workgroup of k_window_search), 64 and 65 map points (a second 64-lane workgroup of the
projection kernel with one live lane), against a resident frame of 200 features; with mvuRight (the stereo gates read
the xr block on the device) and without."""
import ctypes as C

import numpy as np
import pytest

import keyframe_scenes as ks
import projection_scenes as ps
from visual_sgraphs_amd import orb

pytestmark = pytest.mark.gpu
BOUNDS = (0.0, 0.0, 640.0, 480.0)
SIZES = (1, 4, 5, 64, 65)
NFEAT, SEED = 200, 11
U8, I32, F32 = np.uint8, np.int32, np.float32
PTR = {U8: C.POINTER(C.c_uint8), I32: C.POINTER(C.c_int32), F32: C.POINTER(C.c_float)}
ALL, NONE, ALTERNATE = (lambda i: True), (lambda i: False), (lambda i: i % 2 == 0)


def ptr(a):
    return a.ctypes.data_as(PTR[a.dtype.type]) if a is not None else None


def unwritten(n, dtype):
    """An output array filled with a value no entry writes (0x5A in every byte)."""
    return np.frombuffer(b"\x5a" * (n * np.dtype(dtype).itemsize), dtype).copy()


class Scene:
    def __init__(self, stereo):
        rng = np.random.default_rng(SEED)
        self.kps, self.desc = ks.synthetic_keypoints(SEED, n=NFEAT)
        self.ur = None
        if stereo:
            self.ur = np.where(rng.random(NFEAT) < 0.7, self.kps["x"] - rng.uniform(5, 40, NFEAT), -1).astype(F32)
        self.F = orb.Frame(NFEAT + 1)
        self.F.upload(self.kps, self.desc, BOUNDS, u_right=self.ur)
        self.pose = ps.current_pose(SEED)
        self.fields, self.src = ps.map_points(self.kps, self.desc, self.ur, self.pose, 100 + SEED)
        self.mp = ps.store_of(self.fields, np.arange(NFEAT, dtype=I32))
        self.cp = orb.FramePose.make(**self.pose)
        self.last_pose = ps.last_pose_of(self.pose, 2 * ps.MB, SEED)
        self.lp = orb.FramePose.make(**self.last_pose)
        self.sf = (F32(1.2) ** np.arange(8, dtype=F32)).astype(F32)
        self.inv2 = (F32(1) / (self.sf * self.sf)).astype(F32)
        self.order = rng.permutation(NFEAT).astype(I32)  # the points of a call: the first n of these slots
        self.skip_of = (rng.random(NFEAT) < 0.1).astype(U8)
        self.last = {}

    def last_frame(self, n):
        """A resident last frame of n features that observe the call's points (a tenth of them outliers)."""
        if n not in self.last:
            q = self.order[:n]
            lk, ldesc, slots, _ = ps.last_frame_arrays(self.kps, {k: v[q] for k, v in self.fields.items()}, self.src[q],
                                                       self.last_pose, BOUNDS, SEED, extra=0)
            L = orb.Frame(n + 1)
            L.upload(lk, ldesc, BOUNDS)
            self.last[n] = (L, np.where(slots >= 0, q[np.maximum(slots, 0)], -1).astype(I32))
        return self.last[n]


@pytest.fixture(scope="module")
def lib():
    return orb.load_library()


@pytest.fixture(scope="module")
def scenes():
    return {stereo: Scene(stereo) for stereo in (False, True)}


def run(entry, L, s, n, keep, slots="given"):
    """One call of `entry` on the first n points of the scene.  Returns (return value, the required outputs, the optional
    outputs with None where keep(i) is false)."""
    q = np.arange(n, dtype=I32) if slots != "given" else np.ascontiguousarray(s.order[:n])
    slp = ptr(q) if slots != "null" else None
    skip = np.ascontiguousarray(s.skip_of[q])
    F, mp, sf = s.F.handle, s.mp.handle, ptr(s.sf)

    def opt(*dtypes):
        arrays = [unwritten(n, dt) if keep(i) else None for i, dt in enumerate(dtypes)]
        return arrays, [ptr(a) for a in arrays]
    tb, tm = np.zeros(NFEAT, U8), np.full(NFEAT, -1, I32)
    bi, bd = np.zeros(n, I32), np.zeros(n, I32)
    count = C.c_int(-7)
    if entry == "frustum":
        o, op = opt(U8, F32, F32, F32, F32, I32, F32)
        rc = L.vsg_frame_is_in_frustum(F, mp, n, slp, C.byref(s.cp), 0.5, *op)
        return rc, (), o
    if entry == "local":
        o, op = opt(U8, F32, F32)
        rc = L.vsg_frame_search_local_points(F, mp, n, slp, ptr(skip), C.byref(s.cp), 0.5, 3.0, 0.8, 0, 0.0, sf, 8, ptr(tb),
                                             ptr(tm), *op, C.byref(count))
        return rc, (tb, tm, count.value), o
    if entry == "last":
        last, last_slots = s.last_frame(n)
        o, op = opt(U8, F32, F32, F32)
        rc = L.vsg_frame_search_last_frame(F, last.handle, mp, ptr(last_slots), C.byref(s.cp), C.byref(s.lp), ps.MB, 0, 7.0,
                                           sf, 8, 1, ptr(tb), ptr(tm), C.byref(count), *op)
        return rc, (tb, tm, count.value), o
    if entry == "keyframe":
        angle = np.ascontiguousarray(s.kps["angle"][s.src[q]], F32)
        o, op = opt(U8, F32, F32, I32)
        rc = L.vsg_frame_search_keyframe_points(F, mp, n, slp, ptr(skip), C.byref(s.cp), 10.0, 100, sf, 8, 1, ptr(angle),
                                                ptr(tb), ptr(tm), *op)
        return rc, (tb, tm), o
    if entry == "fuse":
        o, op = opt(U8, F32, F32, F32, I32)
        rc = L.vsg_frame_fuse_points(F, mp, n, slp, ptr(skip), C.byref(s.cp), 3.0, sf, ptr(s.inv2), 8, ptr(bi), ptr(bd), *op)
        return rc, (bi, bd), o
    o, op = opt(U8, F32, F32, I32)
    if entry == "fuse_sim3":
        rc = L.vsg_frame_fuse_points_sim3(F, mp, n, slp, ptr(skip), C.byref(s.cp), 4.0, sf, 8, ptr(bi), ptr(bd), *op)
        return rc, (bi, bd), o
    assert entry == "sim3"
    matched = np.full(NFEAT, -1, I32)
    rc = L.vsg_frame_search_sim3_points(F, mp, n, slp, ptr(skip), C.byref(s.cp), 8.0, 1.5, sf, 8, ptr(matched), *op)
    return rc, (matched,), o


def same(a, b):
    return a == b if isinstance(a, int) else (a.dtype == b.dtype and a.tobytes() == b.tobytes())


ENTRIES = ("frustum", "local", "last", "keyframe", "fuse", "fuse_sim3", "sim3")


@pytest.mark.parametrize("stereo", [False, True], ids=["mono", "uright"])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("entry", ENTRIES)
def test_results_do_not_depend_on_which_optional_outputs_are_given(lib, scenes, entry, n, stereo):
    s = scenes[stereo]
    rc, req, full = run(entry, lib, s, n, ALL)
    assert rc >= 0, rc
    assert all((a != unwritten(1, a.dtype)[0]).all() for a in full)  # every entry of every block was copied out
    for name, keep in (("none", NONE), ("alternate", ALTERNATE)):
        rc2, req2, part = run(entry, lib, s, n, keep)
        assert rc2 == rc, name
        assert all(same(a, b) for a, b in zip(req, req2)), name
        assert [a is not None for a in part] == [keep(i) for i in range(len(full))]
        for i, a in enumerate(part):
            assert a is None or same(a, full[i]), (name, i)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("entry", ["frustum", "local"])
def test_a_null_slot_list_is_slots_zero_to_n(lib, scenes, entry, n):
    s = scenes[True]
    rc, req, full = run(entry, lib, s, n, ALL, slots="arange")
    rc2, req2, part = run(entry, lib, s, n, ALTERNATE, slots="null")
    assert rc >= 0 and rc2 == rc
    assert all(same(a, b) for a, b in zip(req, req2))
    for i, a in enumerate(part):
        assert a is None or same(a, full[i]), i


def test_the_scene_exercises_the_searches(lib, scenes):
    """Conditions on the fixture: at 65 points every search finds something, so the required outputs above are not
    all-empty arrays, and the stereo frame's gate has mvuRight to read."""
    s = scenes[True]
    assert (s.ur > 0).sum() > NFEAT // 2
    for entry in ENTRIES[1:]:
        rc, req, full = run(entry, lib, s, 65, ALL)
        print(entry, "returns", rc, "projected", int(full[0].sum()))
        assert rc >= 1 and full[0].sum() >= 10, entry
