"""The host build of csrc/vsg_sim3_opt.h (tests/_sim3optcore) against the NumPy restatement on every scene of
tests/sim3opt_scenes.py -- exact on the return value, the counters and the states, within the measured tolerance on S12 and
chi2 -- and its pieces against libm and the restatement: exp_sim3, Sim3's exponential, product, inverse and map, oplusImpl's
zeroing of the update."""
import math

import numpy as np
import pytest

import sim3opt_hostcore as hc
import sim3opt_reference as sr
import sim3opt_scenes as ss

NAMES = list(ss.scenes())


@pytest.fixture(scope="module")
def host_results():
    return {name: hc.run(s) for name, s in ss.scenes().items()}


@pytest.mark.parametrize("name", NAMES)
def test_host_build_agrees_with_the_restatement(name, host_results):
    got, ref = host_results[name], ss.references()[name]
    assert got["ret"] == ref["ret"]
    for k in hc.COUNTERS:
        assert got[k] == ref[k], (k, got[k], ref[k])
    assert np.array_equal(got["state"], ref["state"])
    d = ss.deviations(ref, dict(S12=got["S12"], chi2={f: tuple(got["chi2"][f]) for f in ref["chi2"]}))
    print(name, d)
    for k, v in d.items():
        assert v <= ss.TOL[k], (k, v, ss.TOL[k])
    for f, c in ref["chi2"].items():
        assert [math.isnan(x) for x in c] == [math.isnan(x) for x in got["chi2"][f]], f
    edge = (got["state"] >= 1) & (got["state"] <= 3)
    assert (got["chi2"][~edge] == hc.SENTINEL_CHI2).all() and set(ref["chi2"]) == set(np.flatnonzero(edge).tolist())


def test_a_return_before_the_update_leaves_the_input_bytes(host_results):
    for name in ("return_zero_after_nulling", "pairs_0", "pairs_1", "pairs_9", "stale_nan"):
        got = host_results[name]
        assert got["ret"] == 0 and got["updated"] == 0 and got["S12_bytes"] == got["input_bytes"], name
    assert host_results["pairs_0"]["more_iterations"] == 5 and (host_results["pairs_0"]["state"] == 0).all()


def test_the_stale_rule_decides_bits_and_values(host_results):
    """The host build against its own FIRST_FRESH variant, which recomputes the errors at the first check (NOT the
    reference): on stale_errors the pairs nulled there carry other bits, on stale_nan NaN against finite values."""
    s, got = ss.scenes()["stale_errors"], host_results["stale_errors"]
    fresh = hc.run(s, first_fresh=True)
    bad = np.flatnonzero(got["state"] == 2)
    assert len(bad) == 10 and np.array_equal(got["state"], fresh["state"])
    assert (got["chi2"][bad] != fresh["chi2"][bad]).any(1).all()
    assert np.abs(got["chi2"][bad] - fresh["chi2"][bad]).max() < 1e-6
    s, got = ss.scenes()["stale_nan"], host_results["stale_nan"]
    fresh = hc.run(s, first_fresh=True)
    cand = ss.candidates(s)
    assert np.isnan(got["chi2"][cand]).all() and (got["state"][cand] == 1).all()
    assert np.isfinite(fresh["chi2"][cand]).all(1).sum() == 8 and (fresh["state"][cand] == 2).any()


def _ulps(a, b):
    return np.abs(a.view(np.int64) - b.view(np.int64))


def _libm_exp(x):
    """math.exp is the C library's exp; numpy.exp is numpy's own vector routine, which is not (it differs from libm on
    about 5 % of a grid on [-1e-8, 1e-8])."""
    return np.array([math.exp(v) for v in x])


def test_exp_against_libm():
    """exp(+-1e-9) decides column 6 of every Jacobian: equal to libm for |x| <= 1e-8, within 1 ulp on [-1, 1]."""
    rng = np.random.default_rng(1)
    tiny = np.concatenate([np.linspace(-1e-8, 1e-8, 20001), rng.uniform(-1e-8, 1e-8, 20000), [1e-9, -1e-9, 0.0, -0.0, 1e-300]])
    assert np.array_equal(hc.exp(tiny), _libm_exp(tiny))
    wide = np.concatenate([np.linspace(-1, 1, 200001), rng.uniform(-1, 1, 100000), [1.0, -1.0, 0.34657359027997264,
                           -0.34657359027997264, np.nextafter(0.34657359027997264, 1), 1e-5, -1e-5]])
    u = _ulps(hc.exp(wide), _libm_exp(wide))
    print("exp_sim3 against libm on [-1, 1]: max %d ulp, %d of %d differ" % (u.max(), (u > 0).sum(), len(u)))
    assert u.max() <= 1
    out = hc.exp(np.array([1.0000001, -1.0000001, np.nan, np.inf, -np.inf, 700.0]))
    assert np.isnan(out).all()


def _close(a, b, tol):
    for x, y in zip(a[:2], b[:2]):
        assert np.abs(np.asarray(x) - np.asarray(y)).max() <= tol, (a, b)
    assert abs(a[2] - b[2]) <= tol * max(1.0, abs(b[2])), (a, b)


def test_sim3_exponential_in_every_branch():
    rng = np.random.default_rng(2)
    for om in (1e-7, 0.3, 2.5):          # theta below and above eps
        for sg in (0.0, 1e-9, 1e-7, 0.2, -0.7):  # |sigma| below and above eps
            a = rng.normal(0, 1, 3)
            u = np.concatenate([a / np.linalg.norm(a) * om, rng.normal(0, 1, 3), [sg]])
            _close(hc.sim3_exp(u), sr.sim3_exp(u), 4e-15)
    one = hc.sim3_exp(np.zeros(7))
    assert one[0].tolist() == [0, 0, 0, 1] and one[1].tolist() == [0, 0, 0] and one[2] == 1.0
    bad = hc.sim3_exp(np.array([0, 0, 0, 1, 1, 1, 2.0]))  # |sigma| > 1: the scale is NaN
    assert math.isnan(bad[2])


def test_sim3_product_inverse_and_map_as_written():
    rng = np.random.default_rng(3)
    for _ in range(20):
        a = sr.sim3(rng.normal(0, 1, 4), rng.normal(0, 1, 3), rng.uniform(0.5, 2))  # quaternions of any norm
        b = sr.sim3(rng.normal(0, 1, 4), rng.normal(0, 1, 3), rng.uniform(0.5, 2))
        x = rng.normal(0, 3, 3)
        for got, want in ((hc.sim3_mul(a, b), sr.sim3_mul(a, b)), (hc.sim3_inverse(a), sr.sim3_inverse(a))):
            for u, v in zip(got[:2], want[:2]):
                assert np.array_equal(u, v)
            assert got[2] == want[2]
        assert np.array_equal(hc.sim3_map(a, x), sr.sim3_map(a, x))
    a = sr.sim3([0, 0, 0, 2.0], [0, 0, 0], 1.0)
    assert hc.sim3_mul(a, a)[0].tolist() == [0, 0, 0, 4.0]  # operator* does not normalise


def test_oplus_zeroes_the_update_in_the_callers_array():
    S = sr.sim3([0, 0, 0, 1], [1, 2, 3], 2.0)
    u = [1e-3, 2e-3, -1e-3, 0.01, 0.02, 0.03, 0.5]
    out, left = hc.oplus(S, u, True)
    assert left[6] == 0 and left[:6].tolist() == u[:6] and out[2] == 2.0
    out, left = hc.oplus(S, u, False)
    assert left[6] == 0.5 and abs(out[2] - 2.0 * math.exp(0.5)) < 1e-15


def test_argument_errors():
    s = ss.scenes()["pairs_64"]
    cand = ss.candidates(s)

    def changed(key, i, v):
        a = s[key].copy()
        a[i] = v
        return {key: a}
    top1 = int(s["kps1"]["octave"][cand].max())
    no_kf2 = changed("idx2", cand[5], -1)
    for over in (changed("slots1", cand[3], s["cap1"]), changed("slots2", cand[3], s["cap2"]),
                 changed("idx2", cand[4], s["n2"]), dict(nlevels=0), dict(nlevels=17), dict(nlevels=top1),
                 dict(no_kf2, all_points=1, **changed("level2", cand[5], 8)),
                 dict(no_kf2, all_points=1, **changed("level2", cand[5], -1)),
                 dict(th2=0.0), dict(th2=-1.0), dict(th2=float("inf")), dict(th2=float("nan"))):
        got = hc.run(s, **over)
        assert got["ret"] == -6 and (got["state"] == hc.SENTINEL_STATE).all() and (got["chi2"] == hc.SENTINEL_CHI2).all(), list(over)
    got = hc.run(s, **dict(no_kf2, **changed("level2", cand[5], 99)))  # never read: all_points = 0 skips the entry
    assert got["ret"] > 0 and got["state"][cand[5]] == 5
