"""The conditions the local-BA scenes of tests/lba_scenes.py rest on, asserted on the restatement (tests/lba_reference.py)
ALONE: the fixture condition that lets every flag of every edge be compared, and what each directed scene is there for."""
import numpy as np
import pytest

import lba_reference as lr
import lba_scenes as ls

NAMES = list(ls.scenes())


def _margin(r):
    with np.errstate(all="ignore"):
        return float(np.min(np.abs(r["chi2"] - r["th"]) / r["th"])) if r["ran"] and len(r["chi2"]) else 1.0


@pytest.mark.parametrize("name", NAMES)
def test_fixture_condition(name):
    """Every compared chi2 stays more than 1e-3 (relative) from its threshold, under N_PERM edge orders too, and the flags,
    counters and stop reason do not depend on the order: the allowed share of excluded edges is zero."""
    ref = ls.references()[name]
    assert ref["ran"] == 1
    assert _margin(ref) > 1e-3
    for p in ls.permuted_references()[name]:
        assert _margin(p) > 1e-3
        assert (p["erase"] == ref["erase"]).all()
        assert (p["depth_positive"] == ref["depth_positive"]).all()
        for k in ("iterations_run", "trials_run", "stop_reason", "n_mono", "n_stereo"):
            assert p[k] == ref[k], k
        assert [[t[1:] for t in it] for it in p["trace"]] == [[t[1:] for t in it] for it in ref["trace"]]


def test_committed_spread_bounds_the_measured_one():
    """lba_scenes.SPREAD is the measured spread (with its stated floors) as committed: a fresh measurement may differ in the
    last digits with another NumPy / BLAS / libm, so it is bounded from both sides by a factor 4 (the rule of
    test_pose_reference.py), not compared for equality."""
    sp = ls.measure()
    floor = dict(q=2.0 ** -52, t=2.0 ** -52, pos_rel=2.0 ** -23, chi2_rel=2.0 ** -52)
    for k, v in sp.items():
        m = max(v, floor[k])
        assert m <= 4 * ls.SPREAD[k] and ls.SPREAD[k] <= 4 * m, (k, v, ls.SPREAD[k])
        assert ls.TOL[k] == 64 * ls.SPREAD[k]


@pytest.mark.parametrize("name", ls.CAP_NAMES)
def test_cap_fixture_condition(name):
    """test_fixture_condition on the scenes of the reduced system at its tile and at its cap."""
    ref = ls.cap_references()[name]
    assert ref["ran"] == 1
    assert _margin(ref) > 1e-3
    for p in ls.cap_permuted_references()[name]:
        assert _margin(p) > 1e-3
        assert (p["erase"] == ref["erase"]).all()
        assert (p["depth_positive"] == ref["depth_positive"]).all()
        for k in ("iterations_run", "trials_run", "stop_reason", "n_mono", "n_stereo"):
            assert p[k] == ref[k], k
        assert [[t[1:] for t in it] for it in p["trace"]] == [[t[1:] for t in it] for it in ref["trace"]]


def test_committed_cap_spread_bounds_the_measured_one():
    """lba_scenes.SPREAD_CAP against a fresh measurement over cap_scenes() alone, by the rule of
    test_committed_spread_bounds_the_measured_one."""
    sp = ls.measure(cap=True)
    floor = dict(q=2.0 ** -52, t=2.0 ** -52, pos_rel=2.0 ** -23, chi2_rel=2.0 ** -52)
    for k, v in sp.items():
        m = max(v, floor[k])
        assert m <= 4 * ls.SPREAD_CAP[k] and ls.SPREAD_CAP[k] <= 4 * m, (k, v, ls.SPREAD_CAP[k])
        assert ls.TOL_CAP[k] == 64 * ls.SPREAD_CAP[k]


def test_cap_scene_sizes():
    """96 rows are three whole tiles of lba::kSolveTile, 102 are six rows more, 768 are the cap; every optimised keyframe has
    edges and every point four observations; and the scenes are not among those SPREAD is measured over."""
    assert list(ls.cap_scenes()) == ["rows_96", "rows_102", "rows_768"] and not set(ls.cap_scenes()) & set(ls.scenes())
    for name, s in ls.cap_scenes().items():
        n_opt = int((s["fixed"] == 0).sum())
        assert 6 * n_opt == int(name[5:]) == 6 * ls.cap_references()[name]["n_opt_kf"]
        assert np.bincount(s["obs_kf"], minlength=len(s["kfs"]))[s["fixed"] == 0].min() >= 3
        assert (np.diff(s["obs_off"]) == 4).all()
        assert ls.cap_references()[name]["iterations_run"] >= 3  # the reduced solve runs several times


def test_scene_sizes():
    sc = ls.scenes()
    count = lambda s, k: int((s["obs_kf"] == k).sum())
    for n in (63, 64, 65):
        s = sc["points_%d_all" % n]
        assert len(s["slots"]) == n and all(count(s, k) == n for k in range(len(s["kfs"])))
    for n in (255, 256, 257):
        assert len(sc["points_%d" % n]["slots"]) == n
    assert len(sc["one_point"]["slots"]) == 1
    s = sc["kf_40"]
    assert int((s["fixed"] == 0).sum()) == 40 and np.diff(s["obs_off"])[0] == 42 and np.diff(s["obs_off"]).max() >= 40
    s = sc["special_vertices"]
    per = np.diff(s["obs_off"])
    assert per[3] == 0 and per[2] == 1
    empty = [k for k in range(len(s["kfs"])) if count(s, k) == 0]
    assert len(empty) == 1 and s["fixed"][empty[0]] == 0
    assert all(s["fixed"][k] for k in s["obs_kf"][s["obs_off"][1]:s["obs_off"][2]])  # point 1: fixed keyframes alone
    assert sc["kf_2_1"]["fixed"][0] == 1 and sc["fixed_last"]["fixed"][0] == 0 and sc["fixed_last"]["fixed"][-1] == 1
    assert all(f["ur"] is None for f in sc["mono_clean"]["kfs"]) and int(sc["mono_clean"]["fixed"].sum()) >= 2
    assert (np.diff(sc["two_observations"]["obs_off"]) == 2).all()
    assert sc["mono_outliers"]["is_out"].mean() > 0.1 and not sc["mono_clean"]["is_out"].any()


def test_special_vertices():
    s, r = ls.scenes()["special_vertices"], ls.references()["special_vertices"]
    empty = [k for k in range(len(s["kfs"])) if not (s["obs_kf"] == k).any()][0]
    assert (r["kf_out"][empty] == s["Tcw"][empty].astype(np.float64)).all()       # no vertex: its input
    assert (r["pos_out"][3] == s["store_pos"][s["slots"][3]]).all()               # an empty list: its bytes
    assert (r["pos_out"][1] != s["store_pos"][s["slots"][1]]).any()               # seen by fixed keyframes alone: it moves
    for k in np.flatnonzero(s["fixed"]):
        assert (r["kf_out"][k] == s["Tcw"][k].astype(np.float64)).all()


def test_first_trial_rejected():
    """kf_2_1: an iteration whose first trial is rejected and a later one accepted (lambda grows in between)."""
    tr = ls.references()["kf_2_1"]["trace"]
    assert any(len(it) > 1 and not it[0][1] and it[-1][1] for it in tr)


def test_ends_by_nbad():
    r = ls.references()["converged_start"]
    assert r["stop_reason"] == lr.STOP_BAD and r["iterations_run"] == 3


def test_ends_by_terminate():
    r = ls.references()["exact_start"]
    assert r["stop_reason"] == lr.STOP_TERMINATE and r["iterations_run"] == 1 and r["trace"][0][-1][0] == 0.0
    assert r["chi2_initial"] == 0.0


def test_stale_errors():
    """The last trial is rejected (rho == 0, Terminate): the compared chi2 is the rejected state's and differs from the one at
    the restored estimates."""
    r = ls.references()["stale_errors"]
    assert r["stop_reason"] == lr.STOP_TERMINATE and not r["trace"][-1][-1][1] and r["chi2_final"] == 400.0
    differ = np.isfinite(r["chi2"]) & (r["chi2"] != r["chi2_fresh"])
    assert differ.sum() >= 20
    for p in ls.permuted_references()["stale_errors"]:
        assert p["stop_reason"] == lr.STOP_TERMINATE and not p["trace"][-1][-1][1]


def test_point_behind_camera():
    r = ls.references()["behind_camera"]
    behind = ~r["depth_positive"]
    assert behind.sum() == 8 and (r["erase"][behind] == 1).all() and (r["chi2"][behind] < 0.5 * r["th"][behind]).all()
    assert r["n_erase"] == 8


def test_non_positive_pivot():
    r = ls.references()["negative_information"]
    assert any(not t[2] for it in r["trace"] for t in it)


def test_returns_before_optimize():
    s = ls.scenes()["kf_2_1"]
    for r in (lr.local_ba(s, stop_flag=True), lr.local_ba(dict(s, fixed=np.zeros_like(s["fixed"]))),
              lr.local_ba(dict(s, obs_off=np.zeros_like(s["obs_off"])))):
        assert r["ran"] == 0 and (r["kf_out"] == s["Tcw"].astype(np.float64)).all()
        assert (r["pos_out"] == s["store_pos"][s["slots"]]).all()
