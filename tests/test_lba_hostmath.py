"""The host build of csrc/vsg_local_ba.h (tests/_localbacore) against the restatement (tests/lba_reference.py): every scene
within the measured tolerance of lba_scenes.py with ALL flags, counters and the stop reason equal; the returns before
optimize; every argument error with nothing written."""
import numpy as np
import pytest

import lba_hostcore as hc
import lba_scenes as ls

NAMES = list(ls.scenes())
INVALID, UNSUPPORTED = -6, -3


def check_against_reference(name, got, cap=False):
    """got: a result in lba_hostcore.result's form (the host build's or the device's).  cap: a scene of cap_scenes(), under
    the tolerance measured over those."""
    s, ref = (ls.cap_scenes()[name], ls.cap_references()[name]) if cap else (ls.scenes()[name], ls.references()[name])
    tol = ls.TOL_CAP if cap else ls.TOL
    assert got["ret"] == 0 and got["ran"] == 1
    for k in ("n_opt_kf", "n_fixed_kf", "n_points", "n_edges", "n_mono", "n_stereo", "n_erase", "iterations_run", "trials_run",
              "stop_reason"):
        assert got[k] == ref[k], k
    assert (got["erase"] == ref["erase"]).all()
    dev = ls.deviations(ref, got)
    for k, v in dev.items():
        assert v <= tol[k], (k, v)
    for k in ("lambda", "chi2_initial", "chi2_final"):
        assert abs(got[k] - ref[k]) <= tol["chi2_rel"] * max(abs(ref[k]), 1e-6), k
    # the store: the listed vertices' positions are the outs, everything else keeps its bytes
    vertex = np.diff(s["obs_off"]) > 0
    expect = s["store_pos"].copy()
    expect[s["slots"][vertex]] = got["pos_out"][vertex]
    assert expect.tobytes() == got["store_pos"].tobytes()


@pytest.mark.parametrize("name", NAMES)
def test_scene(name):
    check_against_reference(name, hc.run(ls.scenes()[name]))


@pytest.mark.parametrize("name", list(ls.CAP_NAMES))
def test_cap_scene(name):
    """The reduced system at whole tiles, one keyframe past them and at its cap of 768 rows."""
    got = hc.run(ls.cap_scenes()[name])
    print(name, ls.deviations(ls.cap_references()[name], got))
    check_against_reference(name, got, cap=True)


def test_stale_rule_decides():
    """Where the stale and the fresh chi2 differ the host build carries the STALE one."""
    ref, got = ls.references()["stale_errors"], hc.run(ls.scenes()["stale_errors"])
    differ = np.flatnonzero(np.isfinite(ref["chi2"]) & (ref["chi2"] != ref["chi2_fresh"]))
    nearer = np.abs(got["chi2"][differ] - ref["chi2"][differ]) < np.abs(got["chi2"][differ] - ref["chi2_fresh"][differ])
    assert len(differ) >= 20 and nearer.mean() > 0.9


def untouched(s, got):
    a = hc.marshal(s)
    return (got["kf_out"] == hc.SENTINEL_F).all() and (got["pos_out"] == hc.SENTINEL_F).all() and \
        (got["erase"] == hc.SENTINEL_ERASE).all() and (got["chi2"] == hc.SENTINEL_F).all() and \
        got["store_pos"].tobytes() == np.ascontiguousarray(s["store_pos"], np.float32).tobytes() and a["K"] >= 0


def error_cases():
    """name -> (overrides / arguments of lba_hostcore.run, the expected return code); shared with the device test."""
    s = ls.scenes()["kf_2_1"]
    E, P = int(s["obs_off"][-1]), len(s["slots"])

    def put(key, i, v):
        a = s[key].copy()
        a[i] = v
        return {key: a}
    twice = s["slots"].copy()
    twice[5] = twice[2]
    deep = [dict(f) for f in s["kfs"]]
    deep[1] = dict(deep[1], octave=deep[1]["octave"].copy())
    deep[1]["octave"][int(s["obs_idx"][np.flatnonzero(s["obs_kf"] == 1)[0]])] = s["nlevels"]
    many = ls.make(701, 129, 1, 150, 10)
    cases = {
        "null_slots": (dict(null=("slots",)), INVALID), "null_obs_off": (dict(null=("obs_off",)), INVALID),
        "null_obs_kf": (dict(null=("obs_kf",)), INVALID), "null_obs_idx": (dict(null=("obs_idx",)), INVALID),
        "null_Tcw": (dict(null=("kf_Tcw",)), INVALID), "null_fixed": (dict(null=("kf_fixed",)), INVALID),
        "null_cam": (dict(null=("kf_cam",)), INVALID), "null_sigma": (dict(null=("inv_level_sigma2",)), INVALID),
        "null_kf_out": (dict(null=("kf_Tcw_out",)), INVALID), "null_erase": (dict(null=("erase",)), INVALID),
        "null_res": (dict(null=("res",)), INVALID),
        "off_not_from_zero": (put("obs_off", 0, 1), INVALID), "off_descends": (put("obs_off", 3, int(s["obs_off"][2]) - 1), INVALID),
        "kf_negative": (put("obs_kf", 4, -1), INVALID), "kf_past_end": (put("obs_kf", 4, len(s["kfs"])), INVALID),
        "idx_negative": (put("obs_idx", E - 1, -1), INVALID),
        "idx_past_end": (put("obs_idx", 0, len(s["kfs"][int(s["obs_kf"][0])]["x"])), INVALID),
        "slot_negative": (put("slots", 1, -1), INVALID), "slot_past_end": (put("slots", P - 1, s["capacity"]), INVALID),
        "slot_twice": (dict(slots=twice), INVALID),
        "nlevels_0": (dict(nlevels=0), INVALID), "nlevels_17": (dict(nlevels=17), INVALID),
        "octave_past_nlevels": (dict(kfs=deep), INVALID),
        "iterations_0": (dict(iterations=0), INVALID), "iterations_101": (dict(iterations=101), INVALID),
        "nleft": (dict(nleft=np.array([-1, 3, -1], np.int32)), UNSUPPORTED),
        "edges_on_fixed_alone": (dict(fixed=np.array([1, 1, 1], np.uint8)), UNSUPPORTED),
    }
    return s, cases, many


@pytest.mark.parametrize("case", list(error_cases()[1]))
def test_argument_error(case):
    s, cases, _ = error_cases()
    kw, code = cases[case]
    scene_over = {k: v for k, v in kw.items() if k not in ("null", "nleft")}
    got = hc.run(s, null=kw.get("null", ()), nleft=kw.get("nleft"), **scene_over)
    assert got["ret"] == code
    if "null" not in kw:
        assert untouched(dict(s, **scene_over), got)
        assert got["res_bytes"] == b"\x5a" * len(got["res_bytes"])


def test_more_than_128_optimised_keyframes():
    _, _, many = error_cases()
    got = hc.run(many)
    assert got["ret"] == UNSUPPORTED and untouched(many, got)


def test_returns_before_optimize():
    s = ls.scenes()["kf_2_1"]
    empty = dict(slots=s["slots"][:0], obs_off=np.zeros(1, np.int32), obs_kf=s["obs_kf"][:0], obs_idx=s["obs_idx"][:0])
    for kw, over in ((dict(stop_flag=1), {}), ({}, dict(fixed=np.zeros(3, np.uint8))), ({}, dict(obs_off=np.zeros_like(s["obs_off"]))),
                     ({}, empty)):
        got = hc.run(s, **kw, **over)
        assert got["ret"] == 0 and got["ran"] == 0 and untouched(dict(s, **over), got)
        assert got["iterations_run"] == 0 and got["n_erase"] == 0
    assert hc.run(s, stop_flag=0)["res_bytes"] == hc.run(s)["res_bytes"]


def test_iterations_argument():
    s = ls.scenes()["kf_3_2"]
    one, ten = hc.run(s, iterations=1), hc.run(s)
    assert one["iterations_run"] == 1 and one["stop_reason"] == 0 and ten["iterations_run"] > 1
    assert one["chi2_initial"] == ten["chi2_initial"] and one["chi2_final"] > ten["chi2_final"]
