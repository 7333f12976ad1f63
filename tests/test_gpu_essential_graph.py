"""vsg_mappoints_optimize_essential_graph and vsg_mappoints_correct_sim3 on the GPU (Optimizer::OptimizeEssentialGraph on
resident map points) against the host build of the same header (tests/_egcore) BIT FOR BIT: return value, res, kf_Scw_out,
world_pos_out, chi2 and the whole store.  Sizes are chosen at the kernels' edges: the 48-column panel of the dense solve
(6 and 7 optimised keyframes: the boundary falls inside a vertex's block), its 64-row tile, 256 threads, the groups of 256
edges of the chi2 tree, a vertex with 300 incident edges, and the cap of 438 optimised keyframes."""
import ctypes as C
import functools
import subprocess
from pathlib import Path

import numpy as np
import pytest

import eg_hostcore as hc
import eg_reference as er
import eg_scenes as es
from test_eg_hostmath import error_cases
from visual_sgraphs_amd import orb

pytestmark = pytest.mark.gpu
U8, F32, I32, F64 = np.uint8, np.float32, np.int32, np.float64
INVALID, UNSUPPORTED = -6, -3
FIELDS = ("world_pos", "normal", "min_dist", "max_dist", "desc", "observed")
ADAPTOR = Path(__file__).resolve().parent / "_adaptor_eg"


class Device:
    """A scene's store on the device, every field of every slot seeded; call() is one raw call of the C entry in the form of
    eg_hostcore.run: sentinels in every out, NULL for the names in `null`; the store is put back first."""

    def __init__(self, s):
        self.s = s
        cap = s["capacity"]
        rng = np.random.default_rng(cap)
        self.fields = dict(world_pos=np.ascontiguousarray(s["store_pos"], F32), normal=rng.normal(0, 1, (cap, 3)).astype(F32),
                           min_dist=rng.uniform(1, 2, cap).astype(F32), max_dist=rng.uniform(5, 9, cap).astype(F32),
                           desc=rng.integers(0, 256, (cap, 32)).astype(U8), observed=rng.integers(0, 2, cap).astype(U8))
        self.mp = orb.MapPoints(cap)
        self.reset()

    def reset(self):
        self.mp.update(np.arange(self.s["capacity"]), **self.fields)

    def store(self):
        return self.mp.read(np.arange(self.s["capacity"]))

    def call(self, null=(), reset=True, no_store=False, n_kf=None, n_edges=None, n_points=None, **over):
        if reset:
            self.reset()
        s = dict(self.s, **over)
        a = hc.marshal(s)
        K, E, P = a["Scw"].shape[0], a["ei"].size, a["slots"].size
        kf_out, pos_out, chi2 = np.full((max(K, 1), 8), hc.SENT), np.full((max(P, 1), 3), hc.SENT, F32), np.full(max(E, 1), hc.SENT)
        res = orb.EssentialGraphResult()
        C.memset(C.addressof(res), 0x5A, C.sizeof(res))
        before = bytes(res)
        ip, fp, bp, dp, sp = C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_double), C.POINTER(orb.Sim3d)
        arg = lambda name, v, t: None if name in null else C.cast(v.ctypes.data_as(C.c_void_p), t)
        rc = orb.load_library().vsg_mappoints_optimize_essential_graph(
            None if (no_store or "store" in null) else self.mp.handle, K if n_kf is None else n_kf, arg("Scw", a["Scw"], sp),
            arg("nonc", a["nonc"], sp), arg("has", a["has"], bp), arg("fixed", a["fixed"], bp), E if n_edges is None else n_edges,
            arg("ei", a["ei"], ip), arg("ej", a["ej"], ip), arg("el", a["el"], bp), int(s["fix_scale"]), int(s["iterations"]),
            P if n_points is None else n_points, arg("slots", a["slots"], ip), arg("ref", a["ref"], ip), arg("kf_out", kf_out, sp),
            arg("pos_out", pos_out, fp), arg("chi2", chi2, dp), None if "res" in null else C.byref(res))
        self.after = self.store()
        out = dict(ret=rc, kf_Scw=kf_out[:K], world_pos=pos_out[:P], chi2=chi2[:E], res_bytes=bytes(res), res_untouched=bytes(res) == before)
        out.update({k: int(getattr(res, k)) for k in hc.RESULT_INTS})
        return out

    def store_untouched(self):
        return all(np.array_equal(self.after[f], self.fields[f]) for f in FIELDS)


def same_bits(dev, got, want, s):
    """Every out and the store, byte for byte; the fields the call does not own keep their bytes."""
    assert got["ret"] == want["ret"]
    assert got["res_bytes"] == want["res_bytes"], ({k: got[k] for k in hc.RESULT_INTS}, {k: want[k] for k in hc.RESULT_INTS})
    assert got["kf_Scw"].tobytes() == want["kf_Scw"].tobytes()
    assert got["chi2"].tobytes() == want["chi2"].tobytes()
    assert got["world_pos"].tobytes() == want["world_pos"].tobytes()
    if want["store_pos"] is not None:
        assert dev.after["world_pos"].tobytes() == want["store_pos"].tobytes()
        assert all(np.array_equal(dev.after[f], dev.fields[f]) for f in FIELDS if f != "world_pos")


@functools.lru_cache(maxsize=None)
def sized_scenes():
    S = es.sized
    out = {"n_opt_%d" % n: S(400 + n, n, covis=2) for n in (1, 6, 7, 10, 37)}
    out["one_edge"] = S(420, 5, n_edges=1)
    for E in (255, 256, 257):
        out["edges_%d" % E] = S(421 + E, 20, n_edges=E)
    out["hub_300"] = S(430, 39, hub=(5, 300))
    for fix in (0, 1):
        for sc in (1.0, 1.3):
            out["fix%d_s%s" % (fix, "1" if sc == 1.0 else "13")] = S(440 + 2 * fix + (sc > 1), 9, covis=1, scale=sc, fix_scale=fix, iterations=3)
    return out


@pytest.mark.parametrize("name", sorted(es.scenes()))
def test_scenes_of_the_cpu_tests_bit_for_bit(name):
    """The seeded loops at both scale drifts and both fix_scale, and the directed scenes: a keyframe without an edge, the
    singular system, a duplicate pair, a fixed-fixed edge, the four branches of log(), the NaN scene."""
    s = es.scenes()[name]
    dev = Device(s)
    same_bits(dev, dev.call(), hc.run(s), s)


@pytest.mark.parametrize("name", sorted(sized_scenes()))
def test_sizes_at_the_kernels_edges_bit_for_bit(name):
    s = sized_scenes()[name]
    dev = Device(s)
    got, want = dev.call(), hc.run(s)
    assert want["ran"] == 1 and want["trials_run"] >= 1
    same_bits(dev, got, want, s)


def test_listed_slots_alone_change():
    s = es.scenes()["loop_fix0_s13"]
    dev = Device(s)
    got = dev.call()
    rest = np.setdiff1d(np.arange(s["capacity"]), s["slots"])
    assert np.array_equal(dev.after["world_pos"][rest].view(np.uint32), dev.fields["world_pos"][rest].view(np.uint32))
    assert np.array_equal(dev.after["world_pos"][s["slots"]].view(np.uint32), got["world_pos"].view(np.uint32))
    assert not np.array_equal(dev.after["world_pos"][s["slots"]], dev.fields["world_pos"][s["slots"]])


def test_no_edges_enqueues_nothing():
    s = es.scenes()["loop_fix0_s1"]
    dev = Device(s)
    none = dict(ei=np.zeros(0, I32), ej=np.zeros(0, I32), eloop=np.zeros(0, U8))
    got, want = dev.call(**none), hc.run(dict(s, **none))
    assert got["ran"] == 0 and got["ret"] == 0 and got["res_bytes"] == want["res_bytes"]
    assert got["kf_Scw"].tobytes() == np.asarray(s["Scw"], F64).tobytes() and (got["world_pos"] == hc.SENT).all()
    assert dev.store_untouched()


def test_pose_graph_alone_with_a_null_store():
    s = es.scenes()["loop_fix0_s13"]
    dev = Device(s)
    none = dict(slots=np.zeros(0, I32), point_ref=np.zeros(0, I32))
    got = dev.call(no_store=True, **none)
    want = hc.run(dict(s, store_pos=None, **none))
    assert got["ret"] == 0 and got["res_bytes"] == want["res_bytes"]
    assert got["kf_Scw"].tobytes() == want["kf_Scw"].tobytes() and got["chi2"].tobytes() == want["chi2"].tobytes()
    assert dev.store_untouched()


def test_at_the_cap():
    """438 optimised + 1 fixed keyframes, a chain with 5 covisibility edges each, 2 iterations: 3066 rows."""
    s = es.sized(450, 438, covis=5, iterations=2, points_per_kf=1)
    dev = Device(s)
    got, want = dev.call(), hc.run(s)
    assert want["n_opt_kf"] == 438 and want["ran"] == 1
    same_bits(dev, got, want, s)


def test_past_the_cap_is_unsupported_and_writes_nothing():
    s = es.sized(451, 439, iterations=1, points_per_kf=1)
    dev = Device(s)
    got = dev.call()
    assert got["ret"] == UNSUPPORTED and got["res_untouched"] and (got["kf_Scw"] == hc.SENT).all() and (got["world_pos"] == hc.SENT).all()
    assert dev.store_untouched()


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_correct_sim3_bit_for_bit(n):
    rng = np.random.default_rng(500 + n)
    cap, R = n + 9, 5
    s = es.sized(460, R - 1)
    pos = rng.uniform(-5, 5, (cap, 3)).astype(F32)
    slots, ref = rng.permutation(cap)[:n].astype(I32), rng.integers(0, R, n).astype(I32)
    to_inv = er.pack(er.s_inv(er.sim3(s["nonc"])))
    dev = Device(dict(capacity=cap, store_pos=pos))
    got = dev.mp.CorrectSim3(slots, ref, s["Scw"], to_inv)
    want = hc.correct(pos, slots, ref, s["Scw"], to_inv)
    after = dev.store()
    assert want["ret"] == 0 and got.tobytes() == want["world_pos"].tobytes()
    assert after["world_pos"].tobytes() == want["store_pos"].tobytes()
    assert all(np.array_equal(after[f], dev.fields[f]) for f in FIELDS if f != "world_pos")


def test_correct_loop_sequence_on_one_store():
    """CorrectLoop: the points of the corrected keyframes through vsg_mappoints_correct_sim3 (LoopClosing.cc:1060-1064), then the
    essential graph on the same store; both against the host build, the second starting from the first's bytes."""
    s = es.scenes()["loop_fix0_s13"]
    dev = Device(s)
    K = len(s["fixed"])
    corrected = np.flatnonzero(s["has"])
    sel = np.flatnonzero(np.isin(s["point_ref"], corrected))
    to_inv = np.array(s["Scw"], F64)
    to_inv[:, :] = er.pack(er.s_inv(er.sim3(s["Scw"])))
    frm = np.where(np.asarray(s["has"], bool)[:, None], s["nonc"], s["Scw"])
    first = dev.mp.CorrectSim3(s["slots"][sel], s["point_ref"][sel], frm, to_inv)
    want1 = hc.correct(s["store_pos"], s["slots"][sel], s["point_ref"][sel], frm, to_inv)
    assert len(sel) > 0 and first.tobytes() == want1["world_pos"].tobytes()
    got = dev.call(reset=False)
    want = hc.run(dict(s, store_pos=want1["store_pos"]))
    same_bits(dev, got, want, s)
    assert K == got["n_kf"]


@pytest.mark.parametrize("case", sorted(error_cases()[1]))
def test_argument_error_then_a_good_call(case):
    """An error returns its code, writes nothing and leaves no kernel behind: the next call on the same thread is right."""
    base, cases = error_cases()
    kw, code = cases[case]
    run_kw = {k: v for k, v in kw.items() if k in ("null", "n_kf", "n_edges", "n_points")}
    dev = Device(base)
    got = dev.call(**run_kw, **{k: v for k, v in kw.items() if k not in run_kw})
    assert got["ret"] == code and got["res_untouched"]
    assert (got["kf_Scw"] == hc.SENT).all() and (got["world_pos"] == hc.SENT).all() and (got["chi2"] == hc.SENT).all()
    assert dev.store_untouched()
    if case in ("null_Scw", "slot_twice", "Scw_nan", "iterations_0"):  # a few are followed up; each follow-up is a whole run
        same_bits(dev, dev.call(), hc.run(base), base)


def test_correct_sim3_errors_write_nothing():
    s = es.scenes()["loop_fix0_s1"]
    dev = Device(s)
    L = orb.load_library()
    sl, ref = np.array(s["slots"], I32), np.array(s["point_ref"], I32)
    a = np.ascontiguousarray(s["Scw"], F64)
    out = np.full((len(sl), 3), hc.SENT, F32)
    ip, fp, sp = C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(orb.Sim3d)
    p = lambda v, t: C.cast(v.ctypes.data_as(C.c_void_p), t)
    dup = sl.copy()
    dup[1] = dup[0]
    bad_ref = ref.copy()
    bad_ref[0] = len(a)
    bad_s = a.copy()
    bad_s[2, 7] = -1.0
    for args in ((None, len(sl), p(sl, ip), p(ref, ip), len(a), p(a, sp), p(a, sp)),
                 (dev.mp.handle, len(sl), None, p(ref, ip), len(a), p(a, sp), p(a, sp)),
                 (dev.mp.handle, len(sl), p(dup, ip), p(ref, ip), len(a), p(a, sp), p(a, sp)),
                 (dev.mp.handle, len(sl), p(sl, ip), p(bad_ref, ip), len(a), p(a, sp), p(a, sp)),
                 (dev.mp.handle, len(sl), p(sl, ip), p(ref, ip), len(a), p(a, sp), p(bad_s, sp)),
                 (dev.mp.handle, -1, p(sl, ip), p(ref, ip), len(a), p(a, sp), p(a, sp))):
        assert L.vsg_mappoints_correct_sim3(*args, p(out, fp)) == INVALID
        assert (out == hc.SENT).all()
    dev.after = dev.store()
    assert dev.store_untouched()


def test_python_method_and_cpp_adaptor_give_the_raw_call(tmp_path):
    s = es.scenes()["duplicate_pair"]
    dev = Device(s)
    raw = dev.call()
    dev.reset()
    got = dev.mp.OptimizeEssentialGraph(s["Scw"], s["nonc"], s["has"], s["fixed"], s["ei"], s["ej"], s["eloop"], s["fix_scale"],
                                        s["slots"], s["point_ref"], s["iterations"])
    assert got["kf_Scw"].tobytes() == raw["kf_Scw"].tobytes() and got["world_pos"].tobytes() == raw["world_pos"].tobytes()
    assert got["chi2"].tobytes() == raw["chi2"].tobytes() and got["trials_run"] == raw["trials_run"]
    subprocess.check_call(["make", "-C", str(ADAPTOR)], stdout=subprocess.DEVNULL)
    a = hc.marshal(s)
    blob = b"".join(np.ascontiguousarray(v).tobytes() for v in (
        np.array([s["capacity"], len(a["fixed"]), len(a["ei"]), len(a["slots"]), s["fix_scale"], s["iterations"]], I32),
        np.asarray(s["store_pos"], F32), a["Scw"], a["nonc"], a["has"], a["fixed"], a["ei"], a["ej"], a["el"], a["slots"], a["ref"]))
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(blob)
    r = subprocess.run([str(ADAPTOR / "eg_check"), str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK %d %d" % (len(a["fixed"]), raw["trials_run"])), (r.returncode, r.stdout, r.stderr[-2000:])
    assert dst.read_bytes() == raw["kf_Scw"].tobytes() + raw["world_pos"].tobytes() + raw["chi2"].tobytes() + \
        dev.after["world_pos"].tobytes()
