"""vsg_frame_optimize_sim3 on the GPU (Optimizer::OptimizeSim3 on two resident keyframes and resident map points) against
the host build of the same header (tests/_sim3optcore) BIT FOR BIT -- return value, res, state and chi2 -- and against
tests/sim3opt_reference.py (the NumPy restatement) under the measured tolerance of tests/sim3opt_scenes.py.  Every scene
of sim3opt_scenes.scenes(); no pair is excluded from any comparison."""
import ctypes as C
import subprocess
import threading
from pathlib import Path

import numpy as np
import pytest

import sim3opt_hostcore as hc
import sim3opt_scenes as ss
from visual_sgraphs_amd import orb

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
ADAPTOR = ROOT / "tests" / "_adaptor_sim3opt"
BOUNDS = (0.0, 0.0, 640.0, 480.0)
U8, F32, I32, F64 = np.uint8, np.float32, np.int32, np.float64
NAMES = list(ss.scenes())
INVALID, UNSUPPORTED = -6, -3  # include/vsg_orb.h: VSG_ERR_INVALID, VSG_ERR_UNSUPPORTED
COUNTERS = hc.COUNTERS


def keypoints(k):
    n = len(k["x"])
    out = np.zeros(n, orb.KP_DTYPE)
    out["x"], out["y"], out["octave"], out["size"], out["angle"] = k["x"], k["y"], k["octave"], 31.0, -1.0
    return out


def frame_pose(p):
    return orb.FramePose.make(p["Rcw"], p["tcw"], np.zeros(3), p["fx"], p["fy"], p["cx"], p["cy"], 40.0, 0.0, 8)


def upload(k):
    n = len(k["x"])
    return orb.Frame(n + 1).upload(keypoints(k), np.zeros((n, 32), U8), BOUNDS)


class Device:
    """A scene's two keyframes and stores on the device."""

    def __init__(self, s):
        self.s = s
        self.kf1, self.kf2 = upload(s["kps1"]), upload(s["kps2"])
        self.mp1 = orb.MapPoints(s["cap1"])
        self.mp1.update(np.arange(s["cap1"]), world_pos=s["pos1"])
        if s["shared"]:
            self.mp2 = self.mp1
        else:
            self.mp2 = orb.MapPoints(s["cap2"])
            self.mp2.update(np.arange(s["cap2"]), world_pos=s["pos2"])
        self.pose1, self.pose2 = frame_pose(s["pose1"]), frame_pose(s["pose2"])

    def call(self):
        s = self.s
        return self.kf1.OptimizeSim3(self.kf2, self.mp1, self.mp2, s["slots1"], s["slots2"], s["idx2"], s["level2"], self.pose1,
                                     self.pose2, s["sig1"], s["sig2"], s["S12"], s["th2"], s["fix_scale"], s["all_points"],
                                     np.full((s["n1"], 2), hc.SENTINEL_CHI2, F64))


@pytest.fixture(scope="module")
def devices():
    return {name: Device(s) for name, s in ss.scenes().items()}


@pytest.fixture(scope="module")
def device_results(devices):
    return {name: d.call() for name, d in devices.items()}


@pytest.fixture(scope="module")
def host_results():
    return {name: hc.run(s) for name, s in ss.scenes().items()}


def same_bits(got, want, what):
    assert got["ret"] == want["ret"], (what, got["ret"], want["ret"])
    for k in COUNTERS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    assert got["state"].tobytes() == want["state"].tobytes(), (what, np.flatnonzero(got["state"] != want["state"])[:8])
    assert got["chi2"].tobytes() == want["chi2"].tobytes(), \
        (what, np.flatnonzero((got["chi2"].view(np.int64) != want["chi2"].view(np.int64)).any(1))[:8])
    assert got["S12_bytes"] == want["S12_bytes"], (what, got["S12"], want["S12"])


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_the_host_build_bit_for_bit(name, device_results, host_results):
    same_bits(device_results[name], host_results[name], name)


@pytest.mark.parametrize("name", NAMES)
def test_device_agrees_with_the_restatement(name, device_results):
    got, ref = device_results[name], ss.references()[name]
    assert got["ret"] == ref["ret"]
    for k in COUNTERS:
        assert got[k] == ref[k], (k, got[k], ref[k])
    assert np.array_equal(got["state"], ref["state"])
    d = ss.deviations(ref, dict(S12=got["S12"], chi2={f: tuple(got["chi2"][f]) for f in ref["chi2"]}))
    print(name, d)
    for k, v in d.items():
        assert v <= ss.TOL[k], (k, v, ss.TOL[k])
    for f, c in ref["chi2"].items():  # the NaN path: NaN where the restatement has NaN
        assert [np.isnan(x) for x in c] == [np.isnan(x) for x in got["chi2"][f]], f
    for a, b in zip(ref["S12"][0].tolist() + ref["S12"][1].tolist() + [ref["S12"][2]],
                    got["S12"][0].tolist() + got["S12"][1].tolist() + [got["S12"][2]]):
        assert np.isnan(a) == np.isnan(b)


def test_a_return_before_the_update_leaves_the_input_bytes(device_results):
    got = device_results["return_zero_after_nulling"]
    assert got["ret"] == 0 and got["updated"] == 0 and got["n_bad"] == 4 and got["more_iterations"] == 10
    assert (got["state"] == 2).sum() == 4 and got["S12_bytes"] == got["input_bytes"]
    assert device_results["pairs_0"]["S12_bytes"] == device_results["pairs_0"]["input_bytes"]
    assert device_results["unnormalised_input"]["updated"] == 1


def test_device_carries_the_stale_errors_at_the_first_check(device_results, host_results):
    """stale_errors: the chi2 of the pairs nulled at the first check are those of the rejected last trial's state -- the
    bits of the host build, which differ from the bits of its variant that recomputes them at the estimate.  stale_nan:
    the first check compares NaN for every pair where the errors at the estimate are finite."""
    s, got = ss.scenes()["stale_errors"], device_results["stale_errors"]
    fresh = hc.run(s, first_fresh=True)
    bad = np.flatnonzero(got["state"] == 2)
    assert len(bad) == 10 and np.array_equal(fresh["state"], got["state"])
    assert got["chi2"][bad].tobytes() == host_results["stale_errors"]["chi2"][bad].tobytes()
    differs = (got["chi2"][bad] != fresh["chi2"][bad]).any(1)
    assert differs.all(), differs
    s, got = ss.scenes()["stale_nan"], device_results["stale_nan"]
    cand = ss.candidates(s)
    fresh = hc.run(s, first_fresh=True)
    assert got["ret"] == 0 and (got["state"][cand] == 1).all() and np.isnan(got["chi2"][cand]).all()
    assert np.isfinite(fresh["chi2"][cand]).all(1).sum() == 8


@pytest.mark.parametrize("name", NAMES)
def test_entries_without_an_edge_keep_their_chi2_bytes(name, device_results):
    got = device_results[name]
    edge = (got["state"] >= 1) & (got["state"] <= 3)
    assert (got["chi2"][~edge] == hc.SENTINEL_CHI2).all()
    assert (got["chi2"][edge] != hc.SENTINEL_CHI2).all()
    assert (got["state"] <= 5).all()


def test_stores_and_frames_are_unchanged_and_a_second_call_is_identical(devices):
    d = devices["pairs_257"]
    before = [d.mp1.read(np.arange(d.mp1.capacity)), d.mp2.read(np.arange(d.mp2.capacity))]
    grids = [d.kf1.grid(), d.kf2.grid()]
    a = d.call()
    b = d.call()
    same_bits(a, b, "second call")
    after = [d.mp1.read(np.arange(d.mp1.capacity)), d.mp2.read(np.arange(d.mp2.capacity))]
    for x, y in zip(before, after):
        for k in x:
            assert x[k].tobytes() == y[k].tobytes(), k
    for g, g2 in zip(grids, [d.kf1.grid(), d.kf2.grid()]):
        for u, v in zip(g, g2):
            assert np.asarray(u).tobytes() == np.asarray(v).tobytes()
    assert a["updated"] == 1


def test_two_threads_on_one_pair_of_stores_give_the_single_thread_bytes(devices, device_results):
    """The scratch is the calling thread's: two threads optimise on the SAME stores and keyframes at the same time."""
    d = devices["kf_1000_300"]
    out, errors = {}, []

    def work(k):
        try:
            out[k] = [d.call() for _ in range(4)]
        except Exception as e:  # noqa: BLE001 -- reported below
            errors.append(e)
        finally:
            orb.load_library().vsg_thread_release()  # the thread's stream and arenas are never freed implicitly
    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for k in range(2):
        for r in out[k]:
            same_bits(r, device_results["kf_1000_300"], "thread %d" % k)


def test_argument_errors_leave_the_outputs_untouched_and_the_next_call_is_right(devices, device_results):
    d = devices["pairs_64"]
    s = d.s
    L = orb.load_library()
    n = s["n1"]
    arr = dict(slots1=np.ascontiguousarray(s["slots1"], I32), slots2=np.ascontiguousarray(s["slots2"], I32),
               idx2=np.ascontiguousarray(s["idx2"], I32), level2=np.ascontiguousarray(s["level2"], I32),
               sig1=np.ascontiguousarray(s["sig1"], F32), sig2=np.ascontiguousarray(s["sig2"], F32))
    S12 = orb.Sim3d.make(*s["S12"])
    ip, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)

    def call(kf1=d.kf1.handle, kf2=d.kf2.handle, mp1=d.mp1.handle, mp2=d.mp2.handle, pose1=d.pose1, pose2=d.pose2, s12=S12,
             nlevels=8, th2=10.0, all_points=0, state=True, res=True, **over):
        a = dict(arr, **over)
        st, chi2, r = np.full(n, 9, U8), np.full(2 * n, -3.0, F64), orb.Sim3OptResult()
        r.n_correspondences = -77

        def ptr(k, t):
            return a[k].ctypes.data_as(t) if a[k] is not None else None
        rc = L.vsg_frame_optimize_sim3(
            kf1, kf2, mp1, mp2, ptr("slots1", ip), ptr("slots2", ip), ptr("idx2", ip), ptr("level2", ip),
            C.byref(pose1) if pose1 is not None else None, C.byref(pose2) if pose2 is not None else None, ptr("sig1", fp),
            ptr("sig2", fp), nlevels, C.byref(s12) if s12 is not None else None, C.c_float(th2), s["fix_scale"], all_points,
            st.ctypes.data_as(C.POINTER(C.c_uint8)) if state else None, chi2.ctypes.data_as(C.POINTER(C.c_double)),
            C.byref(r) if res else None)
        assert (st == 9).all() and (chi2 == -3).all() and r.n_correspondences == -77
        return rc
    cand = ss.candidates(s)

    def changed(key, i, v):
        a = arr[key].copy()
        a[i] = v
        return {key: a}
    lone1 = np.flatnonzero((s["slots1"] >= 0) & (s["slots2"] < 0))[0]  # a slot is checked with or without a partner
    no_kf2 = changed("idx2", cand[5], -1)
    stereo_pair = orb.Frame(8).upload(keypoints(s["kps1"])[:6], np.zeros((6, 32), U8), BOUNDS, nleft=3)
    top1 = int(s["kps1"]["octave"][cand].max())
    cases = [(dict(kf1=None), INVALID), (dict(kf2=None), INVALID), (dict(mp1=None), INVALID), (dict(mp2=None), INVALID),
             (dict(slots1=None), INVALID), (dict(slots2=None), INVALID), (dict(idx2=None), INVALID),
             (dict(level2=None), INVALID), (dict(pose1=None), INVALID), (dict(pose2=None), INVALID),
             (dict(sig1=None), INVALID), (dict(sig2=None), INVALID), (dict(s12=None), INVALID), (dict(state=False), INVALID),
             (dict(res=False), INVALID),
             (changed("slots1", cand[3], s["cap1"]), INVALID), (changed("slots2", cand[3], s["cap2"]), INVALID),
             (changed("slots1", lone1, s["cap1"]), INVALID),
             (changed("idx2", cand[4], s["n2"]), INVALID),
             (dict(nlevels=0), INVALID), (dict(nlevels=17), INVALID),
             (dict(nlevels=top1), INVALID),                                            # an octave of kf1 >= nlevels
             (dict(all_points=1, **dict(no_kf2, level2=changed("level2", cand[5], 8)["level2"])), INVALID),  # level2 used
             (dict(all_points=1, **dict(no_kf2, level2=changed("level2", cand[5], -1)["level2"])), INVALID),
             (dict(th2=0.0), INVALID), (dict(th2=-1.0), INVALID), (dict(th2=float("inf")), INVALID),
             (dict(th2=float("nan")), INVALID),
             (dict(kf1=stereo_pair.handle), UNSUPPORTED), (dict(kf2=stereo_pair.handle), UNSUPPORTED)]
    for kw, code in cases:
        assert call(**kw) == code, list(kw)
        same_bits(d.call(), device_results["pairs_64"], "after %r" % (list(kw),))
    # a level2 outside the table is NOT an error on an entry that never reads it (all_points = 0 skips it)
    bad_level = dict(no_kf2, level2=changed("level2", cand[5], 99)["level2"])
    st, r = np.full(n, 9, U8), orb.Sim3OptResult()
    rc = L.vsg_frame_optimize_sim3(d.kf1.handle, d.kf2.handle, d.mp1.handle, d.mp2.handle, arr["slots1"].ctypes.data_as(ip),
                                   arr["slots2"].ctypes.data_as(ip), bad_level["idx2"].ctypes.data_as(ip),
                                   bad_level["level2"].ctypes.data_as(ip), C.byref(d.pose1), C.byref(d.pose2),
                                   arr["sig1"].ctypes.data_as(fp), arr["sig2"].ctypes.data_as(fp), 8, C.byref(S12),
                                   C.c_float(10.0), s["fix_scale"], 0, st.ctypes.data_as(C.POINTER(C.c_uint8)), None, C.byref(r))
    assert rc >= 0 and st[cand[5]] == 5


def test_cpp_adaptor_gives_the_same_bytes(device_results, tmp_path):
    name = "outliers_fix0_s13"
    s, want = ss.scenes()[name], device_results[name]
    subprocess.check_call(["make", "-C", str(ADAPTOR)], stdout=subprocess.DEVNULL)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"

    def block(a, t):
        a = np.ascontiguousarray(a, t)
        return np.array([a.size], I32).tobytes() + a.tobytes()

    def pose(p):
        return np.concatenate([p["Rcw"], p["tcw"], [p["fx"], p["fy"], p["cx"], p["cy"]]]).astype(F32)
    src.write_bytes(block([s["cap1"], s["cap2"], s["fix_scale"], s["all_points"]], I32) +
                    block(keypoints(s["kps1"]).view(U8), U8) + block(keypoints(s["kps2"]).view(U8), U8) +
                    block(s["pos1"], F32) + block(s["pos2"], F32) + block(s["slots1"], I32) + block(s["slots2"], I32) +
                    block(s["idx2"], I32) + block(s["level2"], I32) + block(pose(s["pose1"]), F32) +
                    block(pose(s["pose2"]), F32) + block(s["sig1"], F32) + block(s["sig2"], F32) +
                    block(np.concatenate([s["S12"][0], s["S12"][1], [s["S12"][2]]]), F64) + block([s["th2"]], F32))
    subprocess.check_call([str(ADAPTOR / "sim3opt_check"), str(src), str(dst)], timeout=120)
    raw = dst.read_bytes()
    n = s["n1"]
    head = np.frombuffer(raw[:8], I32)
    nulled = np.frombuffer(raw[8:8 + n], U8)
    S12 = raw[8 + n:8 + n + 64]
    hess = np.frombuffer(raw[8 + n + 64:8 + n + 64 + 49 * 8], F64)
    assert head.tolist() == [want["ret"], want["n_bad"]]
    assert nulled.tobytes() == ((want["state"] == 2) | (want["state"] == 3)).astype(U8).tobytes()
    assert S12 == want["S12_bytes"]
    assert (hess == 0).all()
