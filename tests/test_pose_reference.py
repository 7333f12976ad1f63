"""tests/pose_reference.py (the NumPy restatement of Optimizer::PoseOptimization that stands in for g2o) checked against
ground truth and for each quirk of the routine it has to keep, and the conditions of the directed scenes of
tests/pose_scenes.py asserted on the restatement alone, before any library call."""
import math

import numpy as np
import pytest

import pose_reference as pr
import pose_scenes as ps

F32 = np.float32


def run(s, **kw):
    return ps.reference(s, **kw)


def ends(r):
    return [log["end"] for log in r["log"]]


def rejected(log):
    return [t for t in log["trials"] if not t[3]]


def test_it_recovers_the_true_pose_on_noise_free_scenes():
    for kind in ("mono", "stereo", "mixed"):
        s = ps.make(401, 90, 80, kind, noise=0.0, start=(0.05, 3.0))
        r = run(s)
        R, t = s["truth"]
        # the observations are float32 pixels of float32 points: 1e-5 px / 500 px focal length ~ 1e-7 rad
        assert np.abs(pr.q_to_matrix(r["q"]) - R).max() < 2e-6 and np.abs(r["t"] - t).max() < 2e-5, kind
        assert r["ret"] == 80 and r["n_bad"] == 0 and r["rounds_run"] == 4


def test_planted_outliers_are_flagged_and_inliers_are_not():
    for name in ("edges_257", "mono_outliers", "stereo_outliers", "frame_1000_300"):
        s, r = ps.scenes()[name], ps.references()[name]
        feats = sorted(r["outlier"])
        assert [r["outlier"][f] for f in feats] == s["is_out"][feats].astype(int).tolist(), name
        assert r["n_bad"] == int(s["is_out"].sum()) > 0 and r["ret"] == r["n_initial"] - r["n_bad"]


def test_round_three_ends_at_a_stationary_point_of_the_plain_inlier_cost():
    s = ps.scenes()["far_start"]
    r = ps.references()["far_start"]
    kps = np.stack([s["kx"], s["ky"]], 1)
    P = pr.Problem(s["feat_slots"], s["world_pos"], kps, s["octave"], s["u_right"], s["cam"], s["inv_sigma2"])
    P.robust = False
    # the edges round 3 optimised over: the inliers of round 2's classification
    inl2 = {f for f, c, th in r["log"][2]["compared"] if not c > th}
    P.outlier = np.array([int(f) not in inl2 for f in P.feat])
    g_end = np.linalg.norm(P.build((r["q"], r["t"]))[1])
    g_start = np.linalg.norm(P.build(pr.est_from_pose(s["q"], s["t"]))[1])
    print("gradient norm: start %.3e, end %.3e" % (g_start, g_end))
    assert g_end < 1e-6 * g_start


def test_lambda_sequence_on_a_hand_worked_case():
    """Three mono edges at the exact pose but for ONE observation moved by one pixel.  lambda0 = 1e-5 * max diag(H); an
    accepted step scales lambda by max(1/3, min(1 - (2 rho - 1)^3, 2/3)); a rejected one multiplies it by ni = 2, 4, ..."""
    s = ps._dyadic()
    keep = np.flatnonzero(s["u_right"] < 0)[:3]
    s["feat_slots"] = np.where(np.isin(np.arange(s["n"]), keep), s["feat_slots"], -1).astype(np.int32)
    s["kx"] = s["kx"].copy()
    s["kx"][keep[0]] += F32(1.0)
    r = run(s)
    assert r["n_initial"] == 3 and r["rounds_run"] == 1          # 3 .. 9 edges: exactly one round
    log = r["log"][0]
    kps = np.stack([s["kx"], s["ky"]], 1)
    P = pr.Problem(s["feat_slots"], s["world_pos"], kps, s["octave"], s["u_right"], s["cam"], s["inv_sigma2"])
    chi0, b, H = P.build(pr.est_from_pose(s["q"], s["t"]))
    assert chi0 == float(s["inv_sigma2"][s["octave"][keep[0]]])  # one pixel, squared, times invSigma2
    assert log["lambda0"] == 1e-5 * max(abs(H[j, j]) for j in range(6))
    lam, ni = log["lambda0"], 2.0
    for it, used, rho, good in log["trials"]:
        assert used == lam, (it, used, lam)
        if good:
            lam *= max(1.0 / 3.0, min(1.0 - math.pow(2 * rho - 1, 3), 2.0 / 3.0))
            ni = 2.0
        else:
            lam *= ni
            ni *= 2
    assert log["trials"][0][3] and log["trials"][0][2] > 0.9        # the first step is a near-perfect Gauss-Newton step
    assert log["trials"][1][1] == log["lambda0"] / 3.0             # so lambda drops by the lower scale


def test_every_round_restarts_from_the_frames_pose():
    s = ps.scenes()["mixed_clean"]
    r = ps.references()["mixed_clean"]
    # no outlier is flagged in this scene, so rounds 0 and 1 solve the same problem from the same start and agree in
    # every trial; had round 1 started from round 0's result its first lambda and cost would differ
    assert r["n_bad"] == 0
    assert r["log"][0]["lambda0"] == r["log"][1]["lambda0"] and r["log"][0]["trials"] == r["log"][1]["trials"]
    assert len(r["log"][0]["trials"]) > 3


def test_huber_kernel_is_dropped_for_round_three():
    """mixed_clean flags nobody, so all four rounds optimise the SAME edges from the same start: rounds 0 .. 2 agree trial
    for trial, round 3 differs from its first lambda on because round 2's classification removed the robust kernel (at
    the start pose, 1 degree off, many residuals lie beyond delta)."""
    r = ps.references()["mixed_clean"]
    assert all(not c > th for log in r["log"] for _, c, th in log["compared"])
    assert r["log"][1]["trials"] == r["log"][2]["trials"] and r["log"][1]["lambda0"] == r["log"][2]["lambda0"]
    assert r["log"][3]["lambda0"] > r["log"][2]["lambda0"]     # rho1 < 1 scaled H down while the kernel was on


def test_float_thresholds_and_deltas():
    assert pr.DELTA[0] == float(F32(math.sqrt(5.991))) != math.sqrt(5.991)
    assert pr.DELTA[1] == float(F32(math.sqrt(7.815))) != math.sqrt(7.815)
    assert float(pr.TH[0]) != 5.991 and float(pr.TH[1]) != 7.815      # 5.991f, 7.815f
    s, r = ps.scenes()["planted"], ps.references()["planted"]
    assert len(s["planted"]) == 8
    for f, factor in s["planted"].items():
        assert r["outlier"][f] == (1 if factor > 1 else 0), (f, factor)
        th = 7.815 if s["u_right"][f] >= 0 else 5.991
        # planted at the TRUE pose; the four 0.8x features pull the optimum a little (4 of 68 inliers), so the value at
        # the converged pose is only near the planted one -- on its side of the threshold is what counts
        assert abs(float(r["chi2"][f]) / th - factor) < 0.2 * factor, (f, factor, r["chi2"][f])
    assert all(c.dtype == F32 for c in r["chi2"].values())


def test_early_ends():
    for name, n in (("edges_0", 0), ("edges_2", 2)):
        s, r = ps.scenes()[name], ps.references()[name]
        assert r["ret"] == 0 and r["rounds_run"] == 0 and r["n_initial"] == n
        assert list(r["outlier"].values()) == [0] * n              # mvbOutlier[i] = false before the return
        assert np.array_equal(r["q"], pr.est_from_pose(s["q"], s["t"])[0])   # no pose change
    for name in ("edges_3", "edges_9"):
        assert ps.references()[name]["rounds_run"] == 1
    assert ps.references()["edges_10"]["rounds_run"] == 4


def test_far_start_rejects_a_trial():
    r = ps.references()["far_start"]
    assert len(rejected(r["log"][0])) >= 1
    # and a rejected trial is followed by lambda * ni
    tr = r["log"][0]["trials"]
    k = next(i for i, t in enumerate(tr[:-1]) if not t[3] and tr[i + 1][0] == t[0])
    assert tr[k + 1][1] >= 2 * tr[k][1]
    # the bad-step sequence pinned to literal factors: within one iteration, consecutive rejections multiply lambda by
    # ni = 2, 4, 8, ... (exact: powers of two)
    last_it = [t for t in tr if t[0] == tr[-1][0]]
    first = next(i for i, t in enumerate(last_it) if not t[3])
    rej = [t for t in last_it[first:]]
    n_rej = next((i for i, t in enumerate(rej) if t[3]), len(rej))
    assert n_rej >= 4, n_rej
    assert [rej[i + 1][1] / rej[i][1] for i in range(n_rej - 1)] == [2.0 ** (i + 1) for i in range(n_rej - 1)]


def test_a_rejected_last_trial_leaves_stale_errors():
    """stale_errors: every optimize() ends with a REJECTED trial (rho == 0 -> Terminate) whose state differs from the
    estimate, so the chi2 that classification compares for inlier edges are those of the rejected state.  On FINITE values:
    the compared float differs from the float at the estimate for at least 100 features."""
    r = ps.references()["stale_errors"]
    for log in r["log"]:
        last = log["trials"][-1]
        assert log["end"] == "rho0" and not last[3] and last[2] == 0.0     # the last trial: rho == 0, rejected
        assert log["trials"][-2][3] and len(log["trials"]) == 2            # after one accepted step
        assert log["stale_differs_float"] >= 100
    st = ps.stale_features(r)
    assert len(st) >= 100 and all(np.isfinite(c) and np.isfinite(f) and c != f for c, f in st.values())
    assert all(r["chi2"][f] == c for f, (c, _) in st.items())              # what was compared is the stale value
    assert ps.follows_stale_rule(r, r["chi2"]) == (len(st), len(st))
    assert ps.follows_stale_rule(r, r["log"][-1]["fresh"])[1] == 0         # a recomputing implementation fails this
    # a qmax end leaves stale errors too, but by then lambda has grown by 2^45 and no compared float moves
    far = ps.references()["far_start"]
    assert far["log"][0]["end"] == "qmax" and far["log"][0]["stale_differs"] > 0


def test_exact_start_terminates_on_rho_zero():
    r = ps.references()["exact_start"]
    assert ends(r) == ["rho0"] * 4 and all(len(log["trials"]) == 1 for log in r["log"])
    assert all(float(c) == 0.0 for c in r["chi2"].values()) and r["n_bad"] == 0


def test_converged_start_ends_by_nbad():
    r = ps.references()["converged_start"]
    assert ends(r) == ["nbad"] * 4


def test_nan_passes_every_comparison():
    s, r = ps.scenes()["z_zero"], ps.references()["z_zero"]
    # a point with camera-frame z == 0 at the input pose poisons every sum: no trial is accepted, ten iterations of one
    # trial each run, the pose stays, and chi2 > th is false for NaN: nobody is flagged
    assert ends(r) == ["iters"] * 4 and all(len(log["trials"]) == 10 for log in r["log"])
    assert all(np.isnan(c) for c in r["chi2"].values()) and r["n_bad"] == 0 and r["ret"] == 24
    assert np.array_equal(r["q"], pr.est_from_pose(s["q"], s["t"])[0]) and np.array_equal(r["t"], np.zeros(3))


def test_plane_step_removals_stay_flagged_and_counted():
    for name, rounds in (("plane_step", 4), ("plane_step_ends_loop", 3)):
        s, r = ps.scenes()[name], ps.references()[name]
        rem = np.flatnonzero((s["removed"] != 0) & (s["feat_slots"] >= 0))
        assert r["held"] == 1 and r["rounds_run"] == rounds
        assert all(r["outlier"][int(f)] == 1 for f in rem) and r["n_bad"] >= len(rem)
        plain = ps.reference(s, hold=False)
        assert plain["n_bad"] < r["n_bad"]
    # without removals the hold changes nothing
    s = ps.scenes()["edges_65"]
    a, b = ps.reference(s, hold=True), ps.references()["edges_65"]
    assert a["held"] == 1 and a["outlier"] == b["outlier"] and np.array_equal(a["q"], b["q"])


def test_fixture_condition():
    """Every compared chi2 is more than 1e-3 (relative) away from its threshold, under 8 edge orders too, and the
    flags, return values and round counts are the same under all of them."""
    for name, ref in ps.references().items():
        runs = [ref] + ps.permuted_references()[name]
        for r in runs:
            assert pr.min_threshold_margin(r) > 1e-3, name
            assert r["outlier"] == ref["outlier"] and r["ret"] == ref["ret"] and r["rounds_run"] == ref["rounds_run"], name


def test_committed_spread_bounds_the_measured_one():
    """pose_scenes.SPREAD is the measured spread (with its stated floors) as committed: a fresh measurement may differ in
    the last digits with another NumPy / libm, so it is bounded from both sides by a factor 4, not compared for equality."""
    sp = ps.measure()
    floor = dict(q=2.0 ** -52, t=2.0 ** -52, chi2_rel=2.0 ** -23)
    for k, v in sp.items():
        m = max(v, floor[k])
        assert m <= 4 * ps.SPREAD[k] and ps.SPREAD[k] <= 4 * m, (k, v, ps.SPREAD[k])
        assert ps.TOL[k] == 64 * ps.SPREAD[k]
