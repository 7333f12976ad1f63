"""The host build of csrc/vsg_pose_opt.h (tests/_posecore, through ctypes) against tests/pose_reference.py on every scene of
tests/pose_scenes.py: flags, return value, n_bad and rounds_run equal; pose and chi2 within pose_scenes.TOL, which is
MEASURED (64 x the restatement's own spread over 8 edge orders), not chosen.  And the header's sin / cos against libm."""
import numpy as np
import pytest

import pose_hostcore as hc
import pose_reference as pr
import pose_scenes as ps

NAMES = list(ps.scenes())


def ulps(a, b):
    return np.abs(a - b) / np.spacing(np.abs(b))


@pytest.mark.parametrize("name", NAMES)
def test_host_build_agrees_with_the_restatement(name):
    s, ref, got = ps.scenes()[name], ps.references()[name], hc.run(ps.scenes()[name])
    for k in ("ret", "n_initial", "n_bad", "rounds_run", "held"):
        assert got[k] == ref[k], (k, got[k], ref[k])
    has = s["feat_slots"] >= 0
    assert got["outlier"][has].tolist() == [ref["outlier"][int(f)] for f in np.flatnonzero(has)]
    assert (got["outlier"][~has] == hc.SENTINEL_FLAG).all() and (got["chi2"][~has] == hc.SENTINEL_CHI2).all()
    d = ps.deviations(ref, dict(q=got["q"], t=got["t"], chi2={f: got["chi2"][f] for f in ref["chi2"]}))
    print(name, d)
    for k, v in d.items():
        assert v <= ps.TOL[k], (k, v, ps.TOL[k])
    for f, c in ref["chi2"].items():
        assert np.isnan(c) == np.isnan(got["chi2"][f])
    if ref["held"]:
        assert np.abs(got["held_q"] - ref["held_q"]).max() <= ps.TOL["q"]
        assert np.abs(got["held_t"] - ref["held_t"]).max() <= ps.TOL["t"]


def test_host_build_keeps_the_stale_errors_of_a_rejected_last_trial():
    """stale_errors: where the restatement's compared (stale) float and the float at the estimate differ, the header's
    chi2 is the stale one.  A header that recomputed the errors at the estimate during classification fails here."""
    ref, got = ps.references()["stale_errors"], hc.run(ps.scenes()["stale_errors"])
    n, stale = ps.follows_stale_rule(ref, got["chi2"])
    assert n >= 100 and stale == n, (n, stale)


def test_hold_and_resume_without_removals_is_the_one_call():
    for name in ("edges_65", "edges_256", "far_start"):
        s = ps.scenes()[name]
        a, b = hc.run(s, hold=True, removed=None), hc.run(s, hold=False)
        assert a["held"] == 1 and b["held"] == 0
        for k in ("ret", "n_bad", "rounds_run"):
            assert a[k] == b[k]
        for k in ("q", "t", "outlier", "chi2"):
            assert a[k].tobytes() == b[k].tobytes(), (name, k)


def test_argument_check():
    s = dict(ps.scenes()["edges_64"])
    bad = s["feat_slots"].copy()
    bad[np.flatnonzero(bad >= 0)[2]] = s["capacity"]
    assert hc.run(dict(s, feat_slots=bad))["ret"] == -6
    assert hc.run(dict(s, nlevels=0))["ret"] == -6 and hc.run(dict(s, nlevels=17))["ret"] == -6
    assert hc.run(dict(s, nlevels=int(s["octave"][s["feat_slots"] >= 0].max())))["ret"] == -6
    r = hc.run(dict(s, feat_slots=bad))
    assert (r["outlier"] == hc.SENTINEL_FLAG).all() and (r["chi2"] == hc.SENTINEL_CHI2).all()   # nothing written


def test_sin_and_cos_within_two_ulp_of_libm():
    rng = np.random.default_rng(5)
    x = np.concatenate([np.linspace(1e-5, np.pi, 100001), rng.uniform(0, np.pi, 100000),
                        10.0 ** rng.uniform(-5, -2, 20000),               # just above SE3Quat::exp's tiny-angle branch
                        np.pi / 2 + rng.uniform(-1e-6, 1e-6, 2000), np.pi - rng.uniform(0, 1e-6, 2000)])
    s, c = hc.sincos(x)
    es, ec = ulps(s, np.sin(x)).max(), ulps(c, np.cos(x)).max()
    print("largest deviation from libm: sin %.2f ulp, cos %.2f ulp" % (es, ec))
    assert es <= 2 and ec <= 2
    s, c = hc.sincos(np.array([np.nan, np.inf, 1e9]))
    assert np.isnan(s).all() and np.isnan(c).all()                       # defined the same on both sides


def test_tiny_angle_branch_of_the_update():
    rng = np.random.default_rng(6)
    q, t = pr.q_normalize(rng.normal(0, 1, 4)), rng.normal(0, 1, 3)
    for scale in (1e-7, 3e-6, 0.0):
        u = np.concatenate([rng.normal(0, 1, 3) * scale, rng.normal(0, 1, 3) * 1e-3])
        assert np.linalg.norm(u[:3]) < 1e-5
        gq, gt = hc.oplus(q, t, u)
        wq, wt = pr.oplus((q, t), u)
        assert np.abs(gq - wq).max() <= 4 * 2.0 ** -52 and np.abs(gt - wt).max() <= 8 * 2.0 ** -52
