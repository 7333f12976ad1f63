"""vsg_frame_pose_optimization / _resume on the GPU (Optimizer::PoseOptimization on a resident frame and resident map
points) against the host build of the same header (tests/_posecore) BIT FOR BIT -- pose, chi2 floats, flags, return value
and res -- and against tests/pose_reference.py (the NumPy restatement) under the measured tolerance of
tests/pose_scenes.py.  Every scene of pose_scenes.scenes(); no feature is excluded from any comparison."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import pose_hostcore as hc
import pose_scenes as ps
from visual_sgraphs_amd import orb

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
ADAPTOR = ROOT / "tests" / "_adaptor_pose"
BOUNDS = (0.0, 0.0, 640.0, 480.0)
U8, F32, I32 = np.uint8, np.float32, np.int32
NAMES = list(ps.scenes())
INVALID, UNSUPPORTED = -6, -3  # include/vsg_orb.h: VSG_ERR_INVALID, VSG_ERR_UNSUPPORTED


def keypoints(s):
    k = np.zeros(s["n"], orb.KP_DTYPE)
    k["x"], k["y"], k["octave"], k["size"], k["angle"] = s["kx"], s["ky"], s["octave"], 31.0, -1.0
    return k


class Device:
    """A scene's frame and store on the device."""

    def __init__(self, s):
        self.s = s
        self.frame = orb.Frame(s["n"] + 1).upload(keypoints(s), np.zeros((s["n"], 32), U8), BOUNDS, u_right=s["u_right"])
        self.mp = orb.MapPoints(s["capacity"])
        self.mp.update(np.arange(s["capacity"]), world_pos=s["world_pos"])

    def call(self, hold=False, feat_slots=None, nlevels=None):
        s = self.s
        sig = s["inv_sigma2"] if nlevels is None else s["inv_sigma2"][:nlevels]
        return self.frame.pose_optimization(self.mp, s["feat_slots"] if feat_slots is None else feat_slots, s["q"], s["t"],
                                            s["cam"], sig, np.full(s["n"], hc.SENTINEL_FLAG, U8), 2 if hold else -1,
                                            np.full(s["n"], hc.SENTINEL_CHI2, F32))

    def run(self):
        """The scene as pose_hostcore.run runs it: held and resumed when it has a removed set."""
        if self.s["removed"] is None:
            return self.call()
        r = self.call(hold=True)
        if not r["held"]:
            return r
        return self.frame.pose_optimization_resume(r["outlier"], self.s["removed"], r["chi2"])


@pytest.fixture(scope="module")
def devices():
    return {name: Device(s) for name, s in ps.scenes().items()}


@pytest.fixture(scope="module")
def device_results(devices):
    return {name: d.run() for name, d in devices.items()}


@pytest.fixture(scope="module")
def host_results():
    return {name: hc.run(s) for name, s in ps.scenes().items()}


def same_bits(got, want, what):
    for k in ("ret", "n_initial", "n_bad", "rounds_run"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    assert got["outlier"].tobytes() == want["outlier"].tobytes(), (what, np.flatnonzero(got["outlier"] != want["outlier"])[:8])
    assert got["chi2"].tobytes() == want["chi2"].tobytes(), (what, np.flatnonzero(got["chi2"].view(I32) != want["chi2"].view(I32))[:8])
    assert got["q"].tobytes() == want["q"].tobytes() and got["t"].tobytes() == want["t"].tobytes(), \
        (what, got["q"] - want["q"], got["t"] - want["t"])


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_the_host_build_bit_for_bit(name, device_results, host_results):
    same_bits(device_results[name], host_results[name], name)


@pytest.mark.parametrize("name", NAMES)
def test_device_agrees_with_the_restatement(name, device_results):
    got, ref = device_results[name], ps.references()[name]
    s = ps.scenes()[name]
    for k in ("ret", "n_initial", "n_bad", "rounds_run"):
        assert got[k] == ref[k], (k, got[k], ref[k])
    has = s["feat_slots"] >= 0
    want = np.array([ref["outlier"][i] for i in np.flatnonzero(has)], U8)
    assert np.array_equal(got["outlier"][has], want)
    d = ps.deviations(ref, dict(q=got["q"], t=got["t"], chi2={f: got["chi2"][f] for f in ref["chi2"]}))
    print(name, d)
    for k, v in d.items():
        assert v <= ps.TOL[k], (k, v, ps.TOL[k])
    for f, c in ref["chi2"].items():  # the NaN path: NaN where the restatement has NaN
        assert np.isnan(c) == np.isnan(got["chi2"][f])


def test_device_keeps_the_stale_errors_of_a_rejected_last_trial(device_results):
    """stale_errors: the chi2 floats are those of the rejected last trial's state, not of the estimate."""
    n, stale = ps.follows_stale_rule(ps.references()["stale_errors"], device_results["stale_errors"]["chi2"])
    assert n >= 100 and stale == n, (n, stale)


@pytest.mark.parametrize("name", NAMES)
def test_features_without_a_slot_keep_their_bytes(name, device_results):
    s, got = ps.scenes()[name], device_results[name]
    none = s["feat_slots"] < 0
    assert (got["outlier"][none] == hc.SENTINEL_FLAG).all() and (got["chi2"][none] == hc.SENTINEL_CHI2).all()
    assert (got["outlier"][~none] <= 1).all()


def test_store_and_frame_are_unchanged_and_a_second_call_is_identical(devices):
    d = devices["edges_257"]
    store, grid = d.mp.read(np.arange(d.mp.capacity)), d.frame.grid()
    a = d.call()
    b = d.call()
    same_bits(a, b, "second call")
    after, grid2 = d.mp.read(np.arange(d.mp.capacity)), d.frame.grid()
    for k in store:
        assert store[k].tobytes() == after[k].tobytes(), k
    for g, g2 in zip(grid, grid2):
        assert np.asarray(g).tobytes() == np.asarray(g2).tobytes()
    assert a["held"] == 0 and a["rounds_run"] == 4


@pytest.mark.parametrize("name", ["edges_65", "edges_256", "far_start", "frame_1000_300"])
def test_hold_and_resume_without_removals_equals_the_one_call(name, devices, device_results, host_results):
    d = devices[name]
    held = d.call(hold=True)
    assert held["held"] == 1 and held["ret"] == 0 and held["rounds_run"] == 2
    h = hc.run(d.s, hold=True, removed=None)
    assert held["q"].tobytes() == h["held_q"].tobytes() and held["t"].tobytes() == h["held_t"].tobytes()
    got = d.frame.pose_optimization_resume(held["outlier"], None, held["chi2"])
    same_bits(got, device_results[name], name)
    assert got["held"] == 0


@pytest.mark.parametrize("name", ["plane_step", "plane_step_ends_loop"])
def test_resume_with_a_removed_set(name, devices, device_results, host_results):
    s, got, ref = ps.scenes()[name], device_results[name], ps.references()[name]
    rem = (s["removed"] != 0) & (s["feat_slots"] >= 0)
    assert rem.sum() >= 4
    assert (got["outlier"][rem] == 1).all()                    # removed features stay flagged ...
    assert got["n_bad"] >= rem.sum() and got["n_bad"] == ref["n_bad"]  # ... and stay counted
    assert got["ret"] == ref["ret"] == got["n_initial"] - got["n_bad"]
    assert got["rounds_run"] == (3 if name == "plane_step_ends_loop" else 4)
    assert got["outlier"][s["feat_slots"] < 0].tolist() == [hc.SENTINEL_FLAG] * int((s["feat_slots"] < 0).sum())


@pytest.mark.parametrize("name", ["edges_0", "edges_2", "edges_3", "edges_9"])
def test_scenes_that_end_before_round_two_are_not_held(name, devices, device_results):
    got = devices[name].call(hold=True)
    assert got["held"] == 0
    same_bits(got, device_results[name], name)
    with pytest.raises(orb.VsgError) as e:
        devices[name].frame.pose_optimization_resume(got["outlier"])
    assert e.value.code == INVALID


def test_resume_needs_a_held_call_on_the_current_features(devices):
    d = Device(ps.scenes()["edges_65"])
    out = np.zeros(d.s["n"], U8)

    def refused():
        with pytest.raises(orb.VsgError) as e:
            d.frame.pose_optimization_resume(out)
        assert e.value.code == INVALID
    refused()                                   # nothing held
    assert d.call(hold=True)["held"] == 1
    d.frame.upload(keypoints(d.s), np.zeros((d.s["n"], 32), U8), BOUNDS, u_right=d.s["u_right"])
    refused()                                   # the features were rewritten
    held = d.call(hold=True)
    d.frame.pose_optimization_resume(held["outlier"])
    refused()                                   # a second resume
    assert d.call(hold=False)["held"] == 0
    refused()                                   # a complete call holds nothing


def test_argument_errors_leave_the_outputs_untouched_and_the_next_call_is_right(devices, device_results):
    d = devices["edges_64"]
    s = d.s
    L = orb.load_library()
    import ctypes as C
    sl = np.ascontiguousarray(s["feat_slots"], I32)
    sig = np.ascontiguousarray(s["inv_sigma2"], F32)
    pose = orb.PoseSE3()
    pose.q[:], pose.t[:] = [float(v) for v in s["q"]], [float(v) for v in s["t"]]
    cam = [float(c) for c in s["cam"]]

    def call(frame=d.frame.handle, mp=d.mp.handle, slots=sl, tcw=pose, sigma=sig, nlevels=8, hold=-1, res=True):
        out, chi2, r = np.full(s["n"], 9, U8), np.full(s["n"], -3, F32), orb.PoseResult()
        r.n_initial = -77
        rc = L.vsg_frame_pose_optimization(
            frame, mp, slots.ctypes.data_as(C.POINTER(C.c_int32)) if slots is not None else None,
            C.byref(tcw) if tcw is not None else None, *cam, sigma.ctypes.data_as(C.POINTER(C.c_float)) if sigma is not None else None,
            nlevels, hold, out.ctypes.data_as(C.POINTER(C.c_uint8)), chi2.ctypes.data_as(C.POINTER(C.c_float)),
            C.byref(r) if res else None)
        assert (out == 9).all() and (chi2 == -3).all() and r.n_initial == -77
        return rc
    too_big = sl.copy()
    too_big[np.flatnonzero(sl >= 0)[3]] = s["capacity"]
    stereo_pair = orb.Frame(8).upload(keypoints(s)[:6], np.zeros((6, 32), U8), BOUNDS, nleft=3)
    for kw, code in ((dict(frame=None), INVALID), (dict(mp=None), INVALID),
                     (dict(slots=None), INVALID), (dict(tcw=None), INVALID),
                     (dict(sigma=None), INVALID), (dict(res=False), INVALID),
                     (dict(slots=too_big), INVALID), (dict(nlevels=0), INVALID),
                     (dict(nlevels=17), INVALID),
                     (dict(nlevels=int(s["octave"][sl >= 0].max())), INVALID),  # an octave >= nlevels
                     (dict(hold=1), INVALID), (dict(hold=3), INVALID),
                     (dict(frame=stereo_pair.handle, slots=sl[:6].copy()), UNSUPPORTED)):
        assert call(**kw) == code, kw
        same_bits(d.call(), device_results["edges_64"], "after %r" % (kw,))


def test_cpp_adaptor_gives_the_same_bytes(devices, device_results, tmp_path):
    name = "plane_step"
    s, want = ps.scenes()[name], device_results[name]
    subprocess.check_call(["make", "-C", str(ADAPTOR)], stdout=subprocess.DEVNULL)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"

    def block(a, t):
        a = np.ascontiguousarray(a, t)
        return np.array([a.size], I32).tobytes() + a.tobytes()
    src.write_bytes(block([s["capacity"]], I32) + block(keypoints(s).view(U8), U8) + block(s["u_right"], F32) +
                    block(s["world_pos"], F32) + block(s["feat_slots"], I32) + block(np.concatenate([s["q"], s["t"]]), F32) +
                    block(s["cam"], F32) + block(s["inv_sigma2"], F32) + block(s["removed"], U8))
    subprocess.check_call([str(ADAPTOR / "pose_check"), str(src), str(dst)], timeout=120)
    raw = dst.read_bytes()
    n = s["n"]
    head = np.frombuffer(raw[:20], I32)
    outlier = np.frombuffer(raw[20:20 + n], U8)
    qt = np.frombuffer(raw[20 + n:20 + n + 28], F32)
    assert head.tolist() == [want["ret"], want["n_initial"], want["n_bad"], want["rounds_run"], 1]
    assert outlier.tobytes() == np.where(s["feat_slots"] >= 0, want["outlier"], 0).astype(U8).tobytes()
    # the adaptor narrows the estimate to the Sophus::SE3f of Optimizer.cc:1447
    assert qt.tobytes() == np.concatenate([want["q"], want["t"]]).astype(F32).tobytes()
