"""vsg_mappoints_global_bundle_adjustment on the GPU (the visual part of Optimizer::BundleAdjustment behind
GlobalBundleAdjustemnt on resident keyframes and resident map points) against the host build of the same headers
(tests/_gbacore) BIT FOR BIT -- return value, res, kf_Tcw_out, world_pos_out, included, chi2 and the store -- and against
tests/gba_reference.py (the NumPy restatement) under the measured tolerance of tests/gba_scenes.py.  Every scene of
gba_scenes.scenes(); no edge or point is excluded from any comparison.  The reduced solve's chain of kernels is tested on
its own against lba::solve_reduced_host, and the whole call against vsg_mappoints_local_bundle_adjustment."""
import ctypes as C
import subprocess
import threading
from pathlib import Path

import numpy as np
import pytest

import gba_hostcore as hc
import gba_scenes as gs
import lba_hostcore as lhc
import lba_scenes as ls
from test_gba_hostmath import check_against_reference, error_cases, over_cap_scene, solver_cases
from test_gpu_local_bundle_adjustment import FIELDS, Device as LocalDevice
from visual_sgraphs_amd import orb

pytestmark = pytest.mark.gpu
ADAPTOR = Path(__file__).resolve().parent / "_adaptor_gba"
U8, F32, I32, F64 = np.uint8, np.float32, np.int32, np.float64
NAMES = list(gs.scenes())
INVALID, UNSUPPORTED = -6, -3  # include/vsg_orb.h: VSG_ERR_INVALID, VSG_ERR_UNSUPPORTED


class Device(LocalDevice):
    """A scene's keyframes and its store on the device; call() is one raw call of the global entry in the form of
    gba_hostcore.run: sentinels in every out, NULL for the names in `null`; the store is put back first."""

    def call(self, stop_flag=None, null=(), reset=True, read=True, flag_array=None, before_call=None, **over):
        if reset:
            self.reset()
        s = dict(self.s, **over)
        a = hc.marshal(s)
        L = orb.load_library()
        handles = (C.c_void_p * max(a["K"], 1))(*[f.handle for f in self.kfs])
        flag = flag_array if flag_array is not None else (None if stop_flag is None else np.array([stop_flag], U8))
        res = orb.GlobalBaResult()  # the binding's own type: test_abi_gba.py holds its layout to the header's
        C.memset(C.addressof(res), 0x5A, C.sizeof(res))
        arg = lambda name, v, t: None if name in null else v.ctypes.data_as(t)
        ip, fp, bp, dp = C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_double)
        if before_call:
            before_call(a)  # the arrays the call is about to write
        rc = L.vsg_mappoints_global_bundle_adjustment(
            self.mp.handle, a["P"], arg("slots", a["slots"], ip), arg("obs_off", a["off"], ip), arg("obs_kf", a["kf"], ip),
            arg("obs_idx", a["idx"], ip), a["K"], handles,
            None if "kf_Tcw" in null else C.cast(a["Tcw"].ctypes.data, C.POINTER(orb.PoseSE3)), arg("kf_fixed", a["fixed"], bp),
            None if "kf_cam" in null else C.cast(a["cam"].ctypes.data, C.POINTER(orb.BaCamera)),
            arg("inv_level_sigma2", a["sig"], fp), s["nlevels"], s["iterations"], int(s["robust"]), int(s["write_store"]),
            None if flag is None else flag.ctypes.data_as(bp),
            None if "kf_Tcw_out" in null else C.cast(a["kf_out"].ctypes.data, C.POINTER(orb.PoseSE3d)),
            arg("world_pos_out", a["pos_out"], fp), arg("included", a["included"], bp), arg("chi2", a["chi2"], dp),
            None if "res" in null else C.byref(res))
        if not read:
            return hc.result(rc, res, a, None)
        self.after = self.store()
        return hc.result(rc, res, a, self.after["world_pos"].copy())


@pytest.fixture(scope="module")
def devices():
    return {name: Device(s) for name, s in gs.scenes().items()}


@pytest.fixture(scope="module")
def device_results(devices):
    return {name: d.call() for name, d in devices.items()}


@pytest.fixture(scope="module")
def host_results():
    return {name: hc.run(s) for name, s in gs.scenes().items()}


def same_bits(got, want, what, store=True):
    assert got["ret"] == want["ret"], (what, got["ret"], want["ret"])
    for k in hc.RES_INTS + hc.RES_DOUBLES:
        assert got[k] == want[k] or (got[k] != got[k] and want[k] != want[k]), (what, k, got[k], want[k])
    assert got["res_bytes"] == want["res_bytes"], what
    for k in ("kf_out", "pos_out", "included", "chi2") + (("store_pos",) if store else ()):
        assert got[k].tobytes() == want[k].tobytes(), (what, k, np.argwhere(got[k] != want[k])[:4])


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_the_host_build_bit_for_bit(name, devices, device_results, host_results):
    same_bits(device_results[name], host_results[name], name)


@pytest.mark.parametrize("name", NAMES)
def test_device_agrees_with_the_restatement(name, device_results):
    print(name, gs.deviations(gs.references()[name], device_results[name]))
    check_against_reference(name, device_results[name])


@pytest.mark.parametrize("name", ("special_vertices", "special_vertices_kept", "rows_114", "rows_150"))
def test_store_after_the_call(name, devices):
    """write_store = 1: the included points' world_pos equals world_pos_out; 0: world_pos keeps its bytes.  Every other slot
    and every other field keeps its bytes in both cases."""
    d = devices[name]
    got = d.call()
    s = d.s
    vertex = np.diff(s["obs_off"]) > 0
    assert got["ran"] == 1 and (got["pos_out"][vertex] != s["store_pos"][s["slots"][vertex]]).any()
    expect = dict(d.fields)
    expect["world_pos"] = d.fields["world_pos"].copy()
    if s["write_store"]:
        expect["world_pos"][s["slots"][vertex]] = got["pos_out"][vertex]
    for k in FIELDS:
        assert d.after[k].tobytes() == np.ascontiguousarray(expect[k]).tobytes(), k
    assert (got["pos_out"][~vertex] == s["store_pos"][s["slots"][~vertex]]).all()
    assert (got["included"] == vertex).all()


# ---- the reduced solve's chain on its own

def test_solver_geometry_is_the_host_build_s():
    assert orb.debug_ba_solver_geometry() == hc.geometry()[:2]


@pytest.mark.parametrize("case", list(solver_cases(gs.PANEL, gs.TILE)))
def test_reduced_solve_equals_the_plain_host_sweep_bit_for_bit(case):
    panel, tile = orb.debug_ba_solver_geometry()
    M, b, compare_x = solver_cases(panel, tile)[case]
    ok_host, x_host = hc.solve(M, b, blocked=False)
    ok_dev, x_dev = orb.debug_ba_reduced_solve(M, b)
    assert ok_dev == ok_host == int(compare_x)
    if compare_x:
        assert x_dev.tobytes() == x_host.tobytes(), np.flatnonzero(x_dev != x_host)[:8]


def test_reduced_solve_reads_the_lower_triangle_alone():
    M, b, _ = solver_cases(gs.PANEL, gs.TILE)["n_%d" % (3 * gs.PANEL + 6)]
    junk = M.copy()
    junk[np.triu_indices(len(b), 1)] = np.nan
    assert orb.debug_ba_reduced_solve(junk, b)[1].tobytes() == orb.debug_ba_reduced_solve(M, b)[1].tobytes()


def test_reduced_solve_argument_errors():
    L = orb.load_library()
    x, ok = np.zeros(4), C.c_int32(7)
    dp = C.POINTER(C.c_double)
    p = x.ctypes.data_as(dp)
    for n, M, b, xo, o in ((0, p, p, p, C.byref(ok)), (6 * hc.geometry()[2] + 1, p, p, p, C.byref(ok)), (2, None, p, p, C.byref(ok)),
                           (2, p, None, p, C.byref(ok)), (2, p, p, None, C.byref(ok)), (2, p, p, p, None)):
        assert L.vsg_debug_ba_reduced_solve(n, M, b, xo, o) == INVALID
    assert ok.value == 7 and (x == 0).all()


# ---- the new call against the local call

def quiet_scene():
    """A scene both calls accept on which the two Huber kernels are the identity: started so near its solution that no
    edge's chi2 ever reaches 5.99, so the calls differ in the reduced solve's schedule alone.  9 optimised keyframes: 54
    rows, a panel and a ragged one."""
    s = gs._with(ls.make(861, 9, 1, 80, 5, start=(0.0005, 0.02)), 1, 1)
    g = gs.gr.Graph(s)
    _, _, _, chi2 = g.errors(g.est, g.X)
    assert chi2.max() < 5.0, chi2.max()
    return s


def test_global_call_equals_the_local_call_bit_for_bit():
    s = quiet_scene()
    dg, dl = Device(s), LocalDevice(s)
    got, want = dg.call(), dl.call()
    assert got["ret"] == want["ret"] == 0 and got["ran"] == want["ran"] == 1 and got["iterations_run"] >= 2
    assert want["chi2"].max() < 5.0 and want["erase"].sum() == 0
    for k in ("kf_out", "pos_out", "chi2", "store_pos"):
        assert got[k].tobytes() == want[k].tobytes(), (k, np.argwhere(got[k] != want[k])[:4])
    for k in hc.RES_INTS + hc.RES_DOUBLES:
        assert got[k] == want[k], k


# ---- arguments, returns, stop flag

def assert_untouched(d, got, included=True):
    assert (got["kf_out"] == hc.SENTINEL_F).all() and (got["pos_out"] == hc.SENTINEL_F).all() and (got["chi2"] == hc.SENTINEL_F).all()
    if included:
        assert (got["included"] == hc.SENTINEL_INCLUDED).all()
    for k in FIELDS:
        assert d.after[k].tobytes() == np.ascontiguousarray(d.fields[k]).tobytes(), k


@pytest.mark.parametrize("case", list(error_cases()[1]))
def test_argument_error_then_a_valid_call(case, devices, device_results):
    """Every error leaves outputs and store untouched, and a second, valid call on the same thread gives the right answer."""
    s, cases = error_cases()
    kw, code = cases[case]
    over = {k: v for k, v in kw.items() if k not in ("null", "nleft")}
    base = devices["mixed_robust_0"]
    d = base if "kfs" not in over and "nleft" not in kw else Device(dict(s, **over), kw.get("nleft"))
    got = d.call(null=kw.get("null", ()), **{k: v for k, v in over.items() if k != "kfs"})
    assert got["ret"] == code
    assert_untouched(d, got)
    if "res" not in kw.get("null", ()):
        assert got["res_bytes"] == b"\x5a" * len(got["res_bytes"])
    same_bits(base.call(), device_results["mixed_robust_0"], "after " + case)


def test_returns_before_optimize(devices):
    d = devices["mixed_robust_0"]
    s = d.s
    empty = dict(slots=s["slots"][:0], obs_off=np.zeros(1, I32), obs_kf=s["obs_kf"][:0], obs_idx=s["obs_idx"][:0])
    for kw, over in ((dict(stop_flag=1), {}), ({}, dict(obs_off=np.zeros_like(s["obs_off"]))), ({}, empty)):
        got = d.call(**kw, **over)
        want = hc.run(s, **kw, **over)
        assert got["ret"] == 0 and got["ran"] == 0
        assert_untouched(d, got, included=False)
        assert got["res_bytes"] == want["res_bytes"] and got["included"].tobytes() == want["included"].tobytes()


def test_no_fixed_keyframe_runs(devices, device_results):
    assert device_results["no_fixed_stereo"]["ran"] == 1 and device_results["no_fixed_stereo"]["n_fixed_kf"] == 0


def test_stop_flag_set_by_a_second_thread_after_the_first_look(devices):
    """`included` is the first out the call writes, after the flag's look on entry and before anything is enqueued.  A second
    thread watches it and sets the flag as soon as it changes: the store lands after the look on entry, while the first
    iterations run.  The call then ends at one of its looks between iterations with stop_reason 3, and its outs are those of
    the host build asked for that many iterations."""
    d = devices["kf_129"]
    s = d.s
    flag, seen, done = np.zeros(1, U8), [], threading.Event()

    def watch(a):
        def body():
            inc = a["included"]
            while not done.is_set():
                if inc[0] != hc.SENTINEL_INCLUDED:
                    flag[0] = 1
                    seen.append(True)
                    return
        t = threading.Thread(target=body)
        t.start()
        seen.append(t)
    try:
        got = d.call(flag_array=flag, before_call=watch)
    finally:
        done.set()
        seen[0].join()
    assert got["ret"] == 0 and got["ran"] == 1 and seen[-1] is True and flag[0] == 1
    full = hc.run(s)
    if got["stop_reason"] != 3:  # the watcher was not scheduled before the last look: nothing to compare but the whole run
        same_bits(got, full, "the flag landed after the last look")
        pytest.fail("the flag never landed between two iterations of a %d-iteration run" % full["iterations_run"])
    assert 1 <= got["iterations_run"] < full["iterations_run"]
    want = hc.run(s, stop_flag=0, stop_after=got["iterations_run"])
    same_bits(got, want, "stopped behind iteration %d" % got["iterations_run"])


def test_more_optimised_keyframes_than_the_cap_is_refused_by_the_library():
    many = over_cap_scene()
    d = Device(many)
    got = d.call()
    assert got["ret"] == UNSUPPORTED and got["res_bytes"] == b"\x5a" * len(got["res_bytes"])
    assert_untouched(d, got)


def test_optional_outs(devices, device_results):
    d = devices["rows_114"]  # write_store = 1
    got, want = d.call(null=("world_pos_out", "chi2")), device_results["rows_114"]
    assert got["ret"] == 0 and got["res_bytes"] == want["res_bytes"]
    assert (got["pos_out"] == hc.SENTINEL_F).all() and (got["chi2"] == hc.SENTINEL_F).all()
    assert got["store_pos"].tobytes() == want["store_pos"].tobytes() and got["kf_out"].tobytes() == want["kf_out"].tobytes()


def test_python_binding(devices, device_results):
    for name in ("rows_54", "rows_48"):
        d = devices[name]
        s = d.s
        d.reset()
        got = d.mp.GlobalBundleAdjustment(s["slots"], s["obs_off"], s["obs_kf"], s["obs_idx"], d.kfs, s["Tcw"], s["fixed"], s["cam"],
                                          s["sig"], iterations=s["iterations"], robust=s["robust"], write_store=s["write_store"])
        want = device_results[name]
        assert got["kf_Tcw"].tobytes() == want["kf_out"].tobytes() and got["world_pos"].tobytes() == want["pos_out"].tobytes()
        assert got["included"].tobytes() == want["included"].tobytes() and got["chi2"].tobytes() == want["chi2"].tobytes()
        assert got["ran"] == 1 and got["stop_reason"] == want["stop_reason"] and got["chi2_final"] == want["chi2_final"]
        assert d.store()["world_pos"].tobytes() == want["store_pos"].tobytes()
    d.reset()
    got = d.mp.GlobalBundleAdjustment(s["slots"], s["obs_off"], s["obs_kf"], s["obs_idx"], d.kfs, s["Tcw"], s["fixed"], s["cam"],
                                      s["sig"], stop_flag=np.array([1], U8))
    assert got["ran"] == 0 and (got["kf_Tcw"] == np.asarray(s["Tcw"], F64)).all() and (got["included"] == 1).all()
    assert (got["world_pos"] == s["store_pos"][s["slots"]]).all()


def _half(s, lo, hi):
    off = s["obs_off"]
    return dict(s, slots=s["slots"][lo:hi], obs_off=(off[lo:hi + 1] - off[lo]).astype(I32), obs_kf=s["obs_kf"][off[lo]:off[hi]],
                obs_idx=s["obs_idx"][off[lo]:off[hi]])


def test_two_threads_on_disjoint_point_sets_of_one_store(devices):
    """The scratch is the calling thread's; each call writes its own points' world_pos alone."""
    d = devices["rows_114"]  # write_store = 1
    d.reset()
    P = len(d.s["slots"])
    halves = [_half(d.s, 0, P // 2), _half(d.s, P // 2, P)]
    want = [hc.run(h) for h in halves]
    out, errors = {}, []

    def work(k):
        try:
            h = halves[k]
            out[k] = d.call(reset=False, read=False, slots=h["slots"], obs_off=h["obs_off"], obs_kf=h["obs_kf"], obs_idx=h["obs_idx"])
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
        same_bits(out[k], want[k], "half %d" % k, store=False)
    final = d.store()["world_pos"]
    expect = d.fields["world_pos"].copy()
    for k in range(2):
        expect[halves[k]["slots"]] = want[k]["pos_out"]
    assert final.tobytes() == expect.tobytes()


@pytest.mark.parametrize("name", ("special_vertices", "mixed_plain_20"))
def test_cpp_adaptor_gives_the_same_bytes(name, device_results, tmp_path):
    s, want = gs.scenes()[name], device_results[name]
    subprocess.check_call(["make", "-C", str(ADAPTOR)], stdout=subprocess.DEVNULL)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"

    def block(a, t, per=1):
        a = np.ascontiguousarray(a, t)
        return np.array([a.size // per], I32).tobytes() + a.tobytes()
    blob = block([s["capacity"], s["iterations"], len(s["kfs"]), s["robust"], s["write_store"]], I32)
    for f in s["kfs"]:
        kps = np.zeros(len(f["x"]), orb.KP_DTYPE)
        kps["x"], kps["y"], kps["octave"], kps["size"], kps["angle"] = f["x"], f["y"], f["octave"], 31.0, -1.0
        blob += np.array([len(kps)], I32).tobytes() + kps.tobytes() + block([] if f["ur"] is None else f["ur"], F32)
    blob += block(s["store_pos"], F32) + block(s["slots"], I32) + block(s["obs_off"], I32) + block(s["obs_kf"], I32) + \
        block(s["obs_idx"], I32) + block(s["Tcw"], F32, 7) + block(s["fixed"], U8) + block(s["cam"], F32, 5) + block(s["sig"], F32)
    src.write_bytes(blob)
    subprocess.check_call([str(ADAPTOR / "gba_check"), str(src), str(dst)], timeout=120)
    raw, at, got = dst.read_bytes(), 0, []
    for size in (56, 4, 1, 8, C.sizeof(orb.GlobalBaResult), 4):
        n = int(np.frombuffer(raw[at:at + 4], I32)[0])
        got.append(raw[at + 4:at + 4 + n * size])
        at += 4 + n * size
    assert at == len(raw)
    assert got[0] == want["kf_out"].tobytes() and got[1] == want["pos_out"].tobytes() and got[2] == want["included"].tobytes()
    assert got[3] == want["chi2"].tobytes() and got[4] == want["res_bytes"] and got[5] == want["store_pos"].tobytes()
