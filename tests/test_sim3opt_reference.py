"""tests/sim3opt_reference.py on its own: the quirks of Optimizer::OptimizeSim3 it keeps (each a directed scene of
tests/sim3opt_scenes.py whose condition is asserted HERE, on the restatement alone), the fixture condition that lets the
other tests compare every flag, and the committed tolerance against a fresh measurement."""
import math

import numpy as np

import sim3opt_reference as sr
import sim3opt_scenes as ss

REFS = ss.references
NAMES = list(ss.scenes())


def test_fixture_condition():
    """Every compared chi2 stays more than 1e-3 (relative) away from th2, and every decision is the same, under every
    member of the perturbation set: no pair needs excluding from a flag comparison."""
    for name, ref in REFS().items():
        assert sr.min_threshold_margin(ref) > 1e-3, name
        for p in ss.perturbed_references()[name]:
            assert sr.min_threshold_margin(p) > 1e-3, name
            assert ss.same_decisions(ref, p), name


def test_committed_spread_bounds_the_measured_one():
    """sim3opt_scenes.SPREAD is the measured spread as committed: a fresh measurement may differ with another NumPy / libm
    (the quantity is rounding noise amplified by 5e8), so it is bounded from both sides by a factor 4, not compared for
    equality."""
    spread, _ = ss.measure()
    for k, v in spread.items():
        m = max(v, 2.0 ** -52)
        assert m <= 4 * ss.SPREAD[k] and ss.SPREAD[k] <= 4 * m, (k, v, ss.SPREAD[k])
        assert ss.TOL[k] == 16 * ss.SPREAD[k]


def test_scenes_cover_what_they_claim():
    sc = ss.scenes()
    for e in (0, 1, 9, 10, 11, 63, 64, 65, 255, 256, 257):
        s = sc["pairs_%d" % e]
        assert len(ss.candidates(s)) == e and REFS()["pairs_%d" % e]["n_correspondences"] == e
        assert s["n1"] > e and (np.diff(ss.candidates(s)) > 1).any() == (e > 1)  # features without a match in between
    s = sc["kf_1000_300"]
    assert s["n1"] == 1000 and len(ss.candidates(s)) == 300 and s["cap1"] == s["cap2"] == 4096 and not s["shared"]
    assert sc["shared_store"]["pos1"] is sc["shared_store"]["pos2"]
    assert {(s["fix_scale"], s["truth"][2]) for s in sc.values()} >= {(0, 1.0), (0, 1.3), (1, 1.0), (1, 1.3)}
    for name in ("all_points_0", "all_points_1"):
        s = sc[name]
        assert (s["idx2"][ss.candidates(s)] < 0).sum() == 30
    # inliers end as inliers, planted outliers are nulled, in every scene built by make() with finite points
    for name, s in sc.items():
        if name in ("stale_nan", "nan_point", "planted", "stale_errors", "exact_start", "z_negative") or name.startswith("all_points"):
            continue
        st = REFS()[name]["state"]
        cand = ss.candidates(s)
        assert ((st[cand] >= 2) == s["is_out"][cand]).all(), name


def test_the_jacobian_is_numeric_and_fix_scale_zeroes_its_last_column():
    for name in ("clean_fix1_s1", "outliers_fix1_s13"):
        log = REFS()[name]["log"]["opt"][0]
        J12, J21 = log["J0"]
        assert (J12[:, :, 6] == 0).all() and (J21[:, :, 6] == 0).all()
        assert (log["H0"][6, :] == 0).all() and (log["H0"][:, 6] == 0).all()  # so H(6, 6) + lambda = lambda
        assert REFS()[name]["S12"][2] == ss.scenes()[name]["S12"][2]           # the scale never moves
    log = REFS()["clean_fix0_s1"]["log"]["opt"][0]
    J12, _ = log["J0"]
    assert (J12[:, :, 6] != 0).any() and log["H0"][6, 6] > 0
    # central differences with delta = 1e-9: entries are multiples of the error's last bits times 5e8, so two columns
    # computed from errors of size ~500 px cannot be finer than about 1e-13 * 5e8
    q = np.abs(J12[np.abs(J12) > 0]).min()
    assert q > 1e-6


def test_oplus_zeroes_the_update_in_the_callers_array():
    u = np.array([1e-3, 2e-3, -1e-3, 0.01, 0.02, 0.03, 0.5])
    S = sr.sim3([0, 0, 0, 1], [1, 2, 3], 2.0)
    out = sr.oplus(S, u, True)
    assert u[6] == 0 and out[2] == 2.0
    u[6] = 0.5
    out = sr.oplus(S, u, False)
    assert u[6] == 0.5 and out[2] == 2.0 * math.exp(0.5)


def test_the_product_does_not_normalise():
    r = REFS()["unnormalised_input"]
    s = ss.scenes()["unnormalised_input"]
    assert abs(np.linalg.norm(s["S12"][0]) - 1.001) < 1e-9
    assert r["updated"] == 1 and abs(np.linalg.norm(r["S12"][0]) - 1.001) < 1e-6
    a = sr.sim3([0, 0, 0, 2.0], [0, 0, 0], 1.0)
    assert sr.sim3_mul(a, a)[0].tolist() == [0, 0, 0, 4.0]


def test_z_negative_and_missing_index_skip_the_entry_and_keep_the_match():
    s, r = ss.scenes()["z_negative"], REFS()["z_negative"]
    assert len(s["z_negative"]) >= 5 and (r["state"][s["z_negative"]] == sr.SKIP_Z).all()
    assert r["n_correspondences"] == len(ss.candidates(s)) - len(s["z_negative"])
    s0, r0, r1 = ss.scenes()["all_points_0"], REFS()["all_points_0"], REFS()["all_points_1"]
    no = ss.candidates(s0)[s0["idx2"][ss.candidates(s0)] < 0]
    assert (r0["state"][no] == sr.SKIP_I2).all() and r0["n_out_kf2"] == 0 and r0["n_correspondences"] == 60
    # with bAllPoints the observation is a NORMALISED coordinate compared with a pixel: every such pair is nulled
    assert r1["n_out_kf2"] == 30 and r1["n_correspondences"] == 90 and (r1["state"][no] == sr.BAD_FIRST).all()
    assert min(r1["chi2"][int(f)][1] for f in no) > 1e3


def test_return_zero_after_nulling():
    s, r = ss.scenes()["return_zero_after_nulling"], REFS()["return_zero_after_nulling"]
    assert r["n_correspondences"] == 12 and r["n_bad"] == 4 and r["ret"] == 0 and r["updated"] == 0
    assert r["more_iterations"] == 10 and len(r["log"]["opt"]) == 1
    assert (r["state"][s["is_out"]] == sr.BAD_FIRST).all() and (r["state"] == sr.BAD_FIRST).sum() == 4
    assert all(np.array_equal(a, b) for a, b in zip(r["S12"][:2], s["S12"][:2])) and r["S12"][2] == s["S12"][2]
    for e, ret in ((9, 0), (10, 10), (11, 11)):
        assert REFS()["pairs_%d" % e]["ret"] == ret


def test_more_iterations():
    a, b = REFS()["no_bad_five_iterations"], REFS()["bad_ten_iterations"]
    assert a["n_bad"] == 0 and a["more_iterations"] == 5 and max(t[0] for t in a["log"]["opt"][1]["trials"]) <= 4
    assert b["n_bad"] == 10 and b["more_iterations"] == 10
    assert "lambda0" in b["log"]["opt"][1] and b["log"]["opt"][1]["trials"][0][0] == 0  # starts again at iteration 0


def test_planted_pairs_fall_on_their_side_of_th2():
    s, r = ss.scenes()["planted"], REFS()["planted"]
    assert sorted(s["planted"].values()) == [0.8] * 4 + [1.25] * 4
    for f, fac in s["planted"].items():
        assert r["state"][f] == (sr.INLIER if fac < 1 else sr.BAD_FIRST), (f, fac)
        k = list(s["planted"]).index(f)
        c = r["log"]["first"][f][0 if k < 4 else 1]      # on either edge alone
        o = r["log"]["first"][f][1 if k < 4 else 0]
        assert abs(c / (fac * ss.TH2) - 1) < 0.1 and o < 0.5, (f, c, o)
    assert r["n_bad"] == 4 and r["ret"] == 68


def test_exact_start_terminates_on_rho_zero():
    r = REFS()["exact_start"]
    for log in r["log"]["opt"]:
        assert log["end"] == "rho0" and len(log["trials"]) == 1 and log["trials"][0][2] == 0.0 and not log["trials"][0][3]
    assert r["ret"] == 24 and all(c == (0.0, 0.0) for c in r["chi2"].values())
    s = ss.scenes()["exact_start"]
    assert all(np.array_equal(a, b) for a, b in zip(r["S12"][:2], s["S12"][:2])) and r["S12"][2] == 1.0


def test_stale_errors_decide_the_first_check():
    r = REFS()["stale_errors"]
    log = r["log"]["opt"][0]
    assert log["end"] == "rho0" and log["trials"][0][3] and not log["trials"][-1][3]  # accepted first, rejected last
    bad = np.flatnonzero(r["state"] == sr.BAD_FIRST)
    assert len(bad) == 10
    for f in bad:
        c12, c21, f12, f21 = r["log"]["first"][int(f)]
        assert (c12, c21) != (f12, f21) and r["chi2"][int(f)] == (c12, c21)  # the output carries the stale values
        assert abs(c12 - f12) < 1e-6
    r = REFS()["stale_nan"]
    assert r["ret"] == 0 and r["n_bad"] == 0 and r["n_correspondences"] == 9
    assert all(not t[3] for t in r["log"]["opt"][0]["trials"]) and len(r["log"]["opt"][0]["trials"]) == 5
    first = r["log"]["first"]
    assert all(math.isnan(v[0]) and math.isnan(v[1]) for v in first.values())
    assert sum(1 for v in first.values() if math.isfinite(v[2]) and math.isfinite(v[3])) == 8


def test_nan_point_is_never_over_the_threshold():
    s, r = ss.scenes()["nan_point"], REFS()["nan_point"]
    f = int(s["feat"][7])
    assert math.isnan(r["chi2"][f][0]) and r["state"][f] == sr.INLIER  # NaN > th2 is false: counted in nIn
    assert r["updated"] == 1 and r["ret"] == 27 and (r["state"] == sr.BAD_SECOND).sum() == 3
    assert all(np.array_equal(a, b) for a, b in zip(r["S12"][:2], s["S12"][:2]))  # no trial was ever accepted


def test_solvers_agree_to_rounding():
    rng = np.random.default_rng(5)
    A = rng.normal(0, 1, (7, 7))
    H, b = A @ A.T + 7 * np.eye(7), rng.normal(0, 1, 7)
    ok1, x1 = sr.solve7(H, b, 0.5, "ldlt")
    ok2, x2 = sr.solve7(H, b, 0.5, "numpy")
    assert ok1 and ok2 and np.abs(x1 - x2).max() < 1e-14
    assert not sr.solve7(-H, b, 0.0)[0]
