"""csrc/vsg_sgraph_ba.h built for the host (tests/_sgbacore) against the NumPy restatement (tests/sgba_reference.py): the
Levenberg decisions, the counters and every flag match exactly, the numbers within the tolerance measured in
tests/sgba_scenes.py; no edge is excluded.  Then the written-out atan2 / sin / cos against libm, Plane3D's oplus / ominus
round trip, the call without planes and rooms against the visual host core bit for bit, and every argument error."""
import ctypes as C
import math

import numpy as np
import pytest

import lba_hostcore as hc
import lba_scenes as ls
import sgba_hostcore as sh
import sgba_reference as sr
import sgba_scenes as ss
from test_lba_hostmath import error_cases as visual_error_cases

NAMES = list(ss.scenes())
INVALID, UNSUPPORTED = -6, -3
F64, I32 = np.float64, np.int32
COUNTERS = ("n_opt_kf", "n_fixed_kf", "n_points", "n_edges", "n_mono", "n_stereo", "n_erase", "iterations_run", "trials_run",
            "stop_reason", "n_planes_active", "n_rooms_active", "n_plane_kf", "n_plane_point", "n_room_edges", "n_rows",
            "n_erase_plane")


def check_against_reference(name, got, big=False):
    """got: a result in sgba_hostcore.result's form (the host build's or the device's)."""
    s, ref = (ss.big_scenes()[name], ss.references(True)[name]) if big else (ss.scenes()[name], ss.references()[name])
    tol = ss.TOL_BIG if big else ss.TOL
    assert got["ret"] == 0 and got["ran"] == ref["ran"]
    if not ref["ran"]:
        return
    for k in COUNTERS:
        assert got[k] == ref[k], k
    assert (got["erase"] == ref["erase"]).all() and (got["erase_plane"] == ref["erase_plane"]).all()
    assert (np.isnan(got["chi2_pk"]) == np.isnan(ref["chi2_pk"])).all() and (np.isnan(got["chi2_pp"]) == np.isnan(ref["chi2_pp"])).all()
    dev = ss.deviations(ref, got)
    for k, v in dev.items():
        assert v <= tol[k], (k, v, tol[k])
    for k in ("lambda", "chi2_initial", "chi2_final"):
        assert abs(got[k] - ref[k]) <= tol["chi2_rel"] * max(abs(ref[k]), 1e-6), k
    vertex = np.diff(s["obs_off"]) > 0
    expect = s["store_pos"].copy()
    expect[s["slots"][vertex]] = got["pos_out"][vertex]
    assert expect.tobytes() == got["store_pos"].tobytes()
    # a plane without an edge is no vertex: its input bytes
    used = np.zeros(len(s["sem"]["plane_eq"]), bool)
    q = s["sem"]
    seen = np.repeat(np.arange(len(used)), np.diff(q["pl_obs_off"]))[(q["w_plane_kf"] > 0) | (q["w_plane_point"] > 0)]
    used[seen] = True
    for r, nw in enumerate(q["room_n_walls"]):
        used[q["room_wall"][r, :nw]] = True
    assert got["plane_out"][~used].tobytes() == np.asarray(q["plane_eq"], F64)[~used].tobytes()


@pytest.mark.parametrize("name", NAMES)
def test_scene(name):
    got = sh.run(ss.scenes()[name])
    print(name, ss.deviations(ss.references()[name], got) if got["ran"] else "ran = 0")
    check_against_reference(name, got)


@pytest.mark.parametrize("name", list(ss.big_scenes()))
def test_big_scene(name):
    got = sh.run(ss.big_scenes()[name])
    print(name, ss.deviations(ss.references(True)[name], got))
    check_against_reference(name, got, big=True)
    if name == "rows_768":
        assert got["n_rows"] == 768


def test_769_rows_or_more_are_unsupported():
    got = sh.run(ss.rows_771())
    assert got["ret"] == UNSUPPORTED
    assert_untouched(got)


@pytest.mark.parametrize("name", ("kf_2_1", "points_257", "special_vertices", "far_start", "stale_errors", "negative_information"))
def test_without_planes_and_rooms_is_the_visual_core_bit_for_bit(name):
    s = ls.scenes()[name]
    got, want = sh.run(ss.no_sem(s)), hc.run(s)
    assert got["ret"] == want["ret"] == 0 and got["res_bytes"][:len(want["res_bytes"])] == want["res_bytes"]
    for k in ("kf_out", "pos_out", "erase", "chi2", "store_pos"):
        assert got[k].tobytes() == want[k].tobytes(), k
    assert got["n_rows"] % 6 == 0 and 0 < got["n_rows"] <= 6 * got["n_opt_kf"] and got["n_planes_active"] == 0


def ulps(a, b):
    if a == b or (a != a and b != b):
        return 0.0
    return abs(a - b) / math.ulp(b) if math.isfinite(a) and math.isfinite(b) and b != 0.0 else math.inf


def test_atan2_against_libm():
    """fdlibm's atan2 is within 2 ulp of the true value and glibc's within 1: at most 3 ulp apart; the special cases exactly."""
    L = sh.lib()
    rng = np.random.default_rng(11)
    inf, nan = math.inf, math.nan
    special = [0.0, -0.0, 1.0, -1.0, inf, -inf, nan, 1e-310, -1e-310, 1e300, -1e300, 0.4375, 0.6875, 1.1875, 2.4375, 2.0 ** 66, 2.0 ** -30]
    worst = 0.0
    for y in special:
        for x in special:
            got, want = L.sgbacore_atan2(y, x), math.atan2(y, x)
            assert ulps(got, want) <= 3 and math.copysign(1, got) == math.copysign(1, want) or (got != got and want != want), (y, x, got, want)
    for scale in (1.0, 1e-3, 1e3, 1e-200, 1e200):
        for y, x in rng.normal(0, 1, (4000, 2)) * [scale, 1.0]:
            worst = max(worst, ulps(L.sgbacore_atan2(y, x), math.atan2(y, x)))
    for r in (0.4375, 0.6875, 1.1875, 2.4375, 1.0):  # around the breakpoints of atan's argument reduction
        for d in rng.uniform(-1e-12, 1e-12, 200):
            for sx, sy in ((1, 1), (-1, 1), (1, -1), (-1, -1)):
                worst = max(worst, ulps(L.sgbacore_atan2(sy * (r + d), sx * 1.0), math.atan2(sy * (r + d), sx * 1.0)))
    print("atan2: worst distance from libm %.2f ulp" % worst)
    assert worst <= 3


def test_sin_cos_of_either_sign_against_libm():
    """pose::sincos_pose is within 2 ulp of libm on [0, pi] (its own test); here over +-1e5 with the signs, and the
    arguments for which both are NaN."""
    L = sh.lib()
    rng = np.random.default_rng(12)
    s, c = C.c_double(), C.c_double()
    worst = 0.0
    for x in list(rng.uniform(-7, 7, 4000)) + list(rng.uniform(-1e5, 1e5, 2000)) + [0.0, -0.0, math.pi, -math.pi, 1e-9, -1e-9]:
        L.sgbacore_sincos(float(x), C.byref(s), C.byref(c))
        for got, want in ((s.value, math.sin(x)), (c.value, math.cos(x))):
            if abs(want) > 1e-3:  # near a zero of the function an ulp of the result is not the measure
                worst = max(worst, ulps(got, want))
            else:
                assert abs(got - want) <= 4 * math.ulp(1.0) * 1e-3 + 4 * math.ulp(abs(x) + 1), (x, got, want)
    print("sin / cos: worst distance from libm %.2f ulp" % worst)
    assert worst <= 2
    for x in (math.inf, -math.inf, math.nan, 1.0001e5, -1.0001e5):
        L.sgbacore_sincos(x, C.byref(s), C.byref(c))
        assert s.value != s.value and c.value != c.value


def _vec(*v):
    return np.array(v, F64)


def test_plane_oplus_then_ominus_round_trip():
    """(p (+) v) (-) p == v up to rounding, over planes of every orientation (the poles and the seam excluded as in the scenes)
    and updates up to 0.3 rad / 0.5 m; the host functions against the restatement's."""
    L = sh.lib()
    rng = np.random.default_rng(13)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    m = sr.Math()
    for _ in range(500):
        c = ss.oblique(rng)
        c[3] = rng.uniform(-6, 6)
        v = rng.uniform(-1, 1, 3) * [0.3, 0.3, 0.5]
        o, e = np.zeros(4), np.zeros(3)
        L.sgbacore_plane_oplus(p(c), p(v), p(o))
        assert abs(np.linalg.norm(o[:3]) - 1) < 1e-15 and np.abs(o - sr.plane_oplus(m, c, v)).max() < 1e-14
        # c.ominus(c.oplus(v)): the new normal in c's frame has azimuth v[0] and elevation v[1]; the distances' difference
        # has the other sign (plane3d.h:83, :94)
        L.sgbacore_plane_ominus(p(c), p(o), p(e))
        assert np.abs(e - sr.plane_ominus(m, c, o)).max() < 1e-13
        assert np.abs(e - _vec(v[0], v[1], -v[2])).max() < 1e-13, (c, v, e)


def test_edge_errors_against_the_restatement():
    L = sh.lib()
    rng = np.random.default_rng(14)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    m = sr.Math()
    for _ in range(200):
        q = rng.normal(0, 1, 4)
        q = q / np.linalg.norm(q) * (1 if q[3] > 0 else -1)
        t, c = rng.normal(0, 2, 3), ss.oblique(rng)
        o = np.zeros(4)
        L.sgbacore_plane_transform(p(q), p(t), p(c), p(o))
        assert np.abs(o - sr.plane_transform((q, t), c)).max() < 1e-14
        pts = np.concatenate([rng.normal(0, 2, (60, 3)), np.ones((60, 1))], 1)
        G = np.ascontiguousarray(pts.T @ pts)
        got, want = L.sgbacore_point_plane_error(p(q), p(t), p(c), p(G)), float(sr.point_plane_error((q, t), c, G)[0])
        assert abs(got - want) <= 1e-12 * max(abs(want), 1.0)
        a, b, v = ss.oblique(rng) * rng.choice([-1, 1]), ss.oblique(rng) * rng.choice([-1, 1]), np.zeros(3)
        L.sgbacore_wall_pair(p(a), p(b), p(v))
        assert np.abs(v - sr.wall_pair(m, a, b)).max() < 1e-14


def assert_untouched(got):
    for k in ("kf_out", "pos_out", "chi2", "plane_out", "room_out", "chi2_pk", "chi2_pp"):
        assert (got[k] == sh.SENTINEL_F).all(), k
    assert (got["erase"] == sh.SENTINEL_ERASE).all() and (got["erase_plane"] == sh.SENTINEL_ERASE).all()
    assert got["res_bytes"] == b"\x5a" * len(got["res_bytes"])


def error_cases():
    """name -> (arguments of sgba_hostcore.run, the expected return code); shared with the device test.  The visual call's
    cases run on the same scene."""
    s = ss.scenes()["two_rooms_shared_wall"]
    q = s["sem"]

    def put(key, i, v):
        a = np.array(q[key], copy=True)
        a.reshape(-1)[i] = v
        return dict(sem={key: a})
    twice = np.array(q["pl_obs_kf"], copy=True)
    twice[1] = twice[0]
    cases = {"null_" + k: (dict(null=(k,)), INVALID) for k in sh.SEM_IN + sh.SEM_OUT[:3]}
    cases.update({
        "plane_off_not_from_zero": (put("pl_obs_off", 0, 1), INVALID),
        "plane_off_descends": (put("pl_obs_off", 2, int(q["pl_obs_off"][1]) - 1), INVALID),
        "plane_kf_negative": (put("pl_obs_kf", 3, -1), INVALID), "plane_kf_past_end": (put("pl_obs_kf", 3, len(s["kfs"])), INVALID),
        "plane_kf_twice": (dict(sem=dict(pl_obs_kf=twice)), INVALID),
        "weight_kf_negative": (put("w_plane_kf", 2, -0.5), INVALID), "weight_kf_nan": (put("w_plane_kf", 2, math.nan), INVALID),
        "weight_point_negative": (put("w_plane_point", 0, -1e-300), INVALID), "weight_point_nan": (put("w_plane_point", 5, math.nan), INVALID),
        "plane_nan": (put("plane_eq", 5, math.nan), INVALID), "plane_inf": (put("plane_eq", 3, math.inf), INVALID),
        "plane_zero_normal": (dict(sem=dict(plane_eq=np.concatenate([[[0.0, 0.0, 0.0, 2.0]], q["plane_eq"][1:]]))), INVALID),
        "walls_3": (put("room_n_walls", 0, 3), INVALID), "walls_0": (put("room_n_walls", 1, 0), INVALID),
        "wall_negative": (put("room_wall", 1, -1), INVALID), "wall_past_end": (put("room_wall", 4, len(q["plane_eq"])), INVALID),
        "wall_twice": (put("room_wall", 3, int(q["room_wall"][0, 0])), INVALID),
    })
    _, visual, _ = visual_error_cases()
    for name, (kw, code) in visual.items():
        if "kfs" not in kw and "nleft" not in kw and "fixed" not in kw and "slots" not in kw and not name.startswith(("off_", "kf_", "idx_", "slot_")):
            cases["visual_" + name] = (kw, code)
    return s, cases


@pytest.mark.parametrize("case", list(error_cases()[1]))
def test_argument_error(case):
    s, cases = error_cases()
    kw, code = cases[case]
    got = sh.run(s, **kw)
    assert got["ret"] == code, case
    if "res" in kw.get("null", ()):
        got["res_bytes"] = b"\x5a"
    assert_untouched(got)


def test_returns_before_optimize():
    s = ss.scenes()["corridor"]
    for kw in (dict(stop_flag=1), dict(fixed=np.zeros(4, np.uint8)), dict(slots=s["slots"][:0], obs_off=np.zeros(1, I32), obs_kf=s["obs_kf"][:0],
                                                                            obs_idx=s["obs_idx"][:0])):
        got = sh.run(s, **kw)
        assert got["ret"] == 0 and got["ran"] == 0 and got["n_rows"] == 0
        for k in ("kf_out", "pos_out", "plane_out", "room_out"):
            assert (got[k] == sh.SENTINEL_F).all(), k
    # room edges are no edges to :2277; plane edges are
    assert sh.run(ss.scenes()["rooms_only_edges"])["ran"] == 0
    got = sh.run(s, obs_off=np.zeros_like(s["obs_off"]))
    assert got["ran"] == 1 and got["n_edges"] == 0 and got["n_plane_point"] > 0
