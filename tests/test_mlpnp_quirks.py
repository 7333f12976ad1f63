"""What MLPnPsolver does that a reader would not expect, each pinned on a directed case: the library (the host build of
csrc/vsg_mlpnp.h) agrees with the restatement AS WRITTEN (tests/mlpnp_reference.py) and differs from a variant of it that
"fixes" the behaviour.  The loop's behaviours are pinned twice where a scene can show them: on directed inlier counts through
mlpnp::select against the loop on counts, and end to end on a scene of groups of correspondences of known sizes."""
import numpy as np

import mlpnp_hostcore as hc
import mlpnp_reference as mr
import mlpnp_scenes as ms

U8, I32 = np.uint8, np.int32


def on_counts(c, first, n_it, max_its, min_inliers, variant, best_set_count=None):
    """select, the loop as written, and the loop with `variant`: the first two agree, the third differs."""
    got = hc.select(np.array(c, I32), first, n_it, max_its, min_inliers)
    want = mr.loop_on_counts(c, first, n_it, max_its, min_inliers)
    fixed = mr.loop_on_counts(c, first, n_it, max_its, min_inliers, variant, best_set_count)
    assert got == want and got != fixed, (got, want, fixed)
    return got


def groups(sizes, order=None):
    s = ms.group_scene(sizes, order)
    rp = mr.make_points(ms.CAM, s["kx"], s["ky"], s["octave"], s["world_pos"], s["slots"], ms.LEVEL_SIGMA2, ms.TH2)
    return s, rp


def end_to_end(s, rp, min_inliers, max_its, n_it, variant):
    """The first call on a scene: the library, the solver as written, the solver with `variant`."""
    got = hc.ransac(s, ms.CAM, ms.LEVEL_SIGMA2, ms.TH2, min_inliers, max_its, 0, n_it)["res"]
    out = []
    for v in (None, variant):
        solver = mr.Solver(rp, s["sets"], min_inliers, max_its, v)
        w = solver.iterate(n_it)
        out.append((int(w["found"]), int(w["no_more"]), int(w["refined"]), solver.iterations, w["n_inliers"]))
    lib = (got["found"], got["no_more"], got["refined"], got["iterations"], got["n_inliers"])
    assert lib == out[0] and lib != out[1], (lib, out)
    return got


def test_the_gate_is_not_strict_the_success_test_is():
    # 8 inliers at min_inliers 8 pass the gate (>=) and become the best; their refinement (8, not MORE than 8) fails
    r = on_counts([8], 0, 1, 1, 8, "gate_strict")
    assert r["found"] and r["best"] == 0
    s, rp = groups((8, 20))
    r = end_to_end(s, rp, 8, 1, 1, "gate_strict")
    assert r["found"] and not r["refined"] and r["no_more"] and r["n_inliers"] == 8


def test_refine_solves_over_the_best_set_and_never_installs_the_pose():
    """Refine() (:303-362) runs computePose over the best set into a local `result` and leaves mRi / mti alone, so its
    CheckInliers() counts hypothesis k's inliers again: success iff c[k] > min_inliers, and the pose, flags and count returned
    are hypothesis k's.  The variant installs the solved pose, as the routine's name promises."""
    # the best set's solve would count 20 inliers: irrelevant, 8 of hypothesis 0 are not MORE than 8
    r = on_counts([8, 7], 0, 2, 2, 8, "refine_installs", best_set_count=[20, 0])
    assert r["found"] and not r["refined"] and r["pose"] == 0
    # a resumed call: hypothesis 1 is no record, the best stays 0, and what is returned is hypothesis 1
    r = on_counts([12, 10], 1, 1, 1, 8, "refine_installs", best_set_count=[8, 0])
    assert r["found"] and r["refined"] and r["best"] == 0 and r["pose"] == 1 and r["iterations"] == 2
    # end to end on a noisy scene: the returned pose is hypothesis k's to the bit, not the solve over its inliers
    s = ms.make(ms.SEEDS[1] + 100, n=100, n_hyp=40)
    rp = mr.make_points(ms.CAM, s["kx"], s["ky"], s["octave"], s["world_pos"], s["slots"], ms.LEVEL_SIGMA2, ms.TH2)
    mi, mx = hc.parameters(0.99, 10, 300, 6, 0.5, 100)
    got = hc.ransac(s, ms.CAM, ms.LEVEL_SIGMA2, ms.TH2, mi, mx, 0, 5)
    res = got["res"]
    assert res["found"] and res["refined"]
    k = res["iterations"] - 1
    assert np.array_equal(res["Tcw"][:3], got["hyp_T"][k].astype(np.float32)) and res["n_inliers"] == got["hyp_inliers"][k]
    pts = hc.points(s, ms.CAM, ms.LEVEL_SIGMA2, ms.TH2)
    assert np.array_equal(got["inlier"][s["where"]].astype(bool), hc.hypotheses(pts, ms.CAM, s["sets"][k:k + 1])["flags"][0])
    written, fixed = mr.Solver(rp, s["sets"], mi, mx), mr.Solver(rp, s["sets"], mi, mx, "refine_installs")
    w, f = written.iterate(5), fixed.iterate(5)
    assert w["found"] and written.iterations == k + 1 and written.refines >= 1  # the solve runs, its result is dropped
    assert np.abs(res["Tcw"] - w["T"]).max() <= 1e-6 and np.abs(res["Tcw"] - f["T"]).max() > 1e-4


def test_the_first_maximum_stays_on_tied_counts():
    r = on_counts([8, 8, 7], 0, 3, 3, 8, "last_max")
    assert r["best"] == 0
    s, rp = groups((9, 9), order=(0, 1))  # at min_inliers 9 neither count is MORE than 9: no return before the end
    got = hc.ransac(s, ms.CAM, ms.LEVEL_SIGMA2, ms.TH2, 9, 2, 0, 2)
    assert list(got["hyp_inliers"]) == [9, 9] and got["res"]["best_hypothesis"] == 0 and got["res"]["n_records"] == 1
    assert got["inlier"][s["where"][:9]].all() and not got["inlier"][s["where"][9:]].any()  # the flags of hypothesis 0


def test_the_exponent_of_epsilon_is_three():
    assert hc.parameters(0.99, 10, 300, 6, 0.5, 100) == mr.ransac_parameters(0.99, 10, 300, 6, 0.5, 100) == (50, 35)
    assert int(np.ceil(np.log(0.01) / np.log(1 - 0.5 ** 6))) == 293  # what the minimal set of 6 would ask for


def test_the_loop_condition_is_an_or():
    # the first call walks max_its although n_iterations is 5; a resumed call walks 5 past max_its
    c = [0] * 20
    assert on_counts(c, 0, 5, 12, 8, "and_loop")["iterations"] == 12
    assert on_counts(c, 12, 5, 12, 8, "and_loop")["iterations"] == 17
    s, rp = groups((7, 7, 7, 7, 7, 7, 7, 7))
    r = end_to_end(s, rp, 8, 8, 5, "and_loop")
    assert r["iterations"] == 8 and r["no_more"] and not r["found"]


def test_no_more_stays_clear_on_a_converged_return_at_the_last_hypothesis():
    r = on_counts([0, 0, 9], 0, 3, 3, 8, "no_more_at_last")
    assert r["found"] and r["refined"] and not r["no_more"] and r["iterations"] == 3
    s, rp = groups((7, 7, 12))
    r = end_to_end(s, rp, 8, 3, 3, "no_more_at_last")
    assert r["found"] and r["refined"] and not r["no_more"] and r["iterations"] == 3


def test_the_no_more_return_is_the_unrefined_pose():
    r = on_counts([9, 0], 0, 2, 2, 9, "refined_on_no_more")
    assert r["found"] and not r["refined"] and r["no_more"]
    s, rp = groups((9, 7))
    got = hc.ransac(s, ms.CAM, ms.LEVEL_SIGMA2, ms.TH2, 9, 2, 0, 2)
    assert got["res"]["found"] and not got["res"]["refined"] and got["res"]["no_more"]
    assert np.array_equal(got["res"]["Tcw"][:3], got["hyp_T"][0].astype(np.float32))  # hypothesis 0's pose, not a refinement's


def test_check_inliers_has_no_depth_test():
    s = ms.make(31, n=40, outliers=0.0, noise=0.0, n_hyp=1)
    i = 7  # mirrored through the camera centre: the same pixel, behind the camera
    Xw = s["world_pos"][s["slots"][s["where"][i]]].astype(np.float64)
    Xc = s["Rcw"] @ Xw + s["tcw"]
    s["world_pos"][s["slots"][s["where"][i]]] = (s["Rcw"].T @ (-Xc - s["tcw"])).astype(np.float32)
    s["sets"] = np.array([[0, 1, 2, 3, 4, 5]], I32)
    pts = hc.points(s, ms.CAM, ms.LEVEL_SIGMA2, ms.TH2)
    rp = mr.make_points(ms.CAM, s["kx"], s["ky"], s["octave"], s["world_pos"], s["slots"], ms.LEVEL_SIGMA2, ms.TH2)
    H = hc.hypotheses(pts, ms.CAM, s["sets"])
    R, t, _ = mr.compute_pose(rp["f"][:6], rp["X"][:6])
    assert (R @ rp["X"][i] + t)[2] < 0  # behind the camera
    assert H["flags"][0, i] and mr.check_inliers(rp, R, t)[0][i] and not mr.check_inliers(rp, R, t, depth_test=True)[0][i]
    assert H["counts"][0] == 40


def test_acos_of_a_trace_out_of_range_gives_omega_zero():
    # a half turn whose trace rounding pushed below -1: acos is NaN, `wnorm > eps` is false, omega stays 0; clamping the
    # argument would make it pi / (2 sin pi) times the antisymmetric part
    R = np.diag([1.0, -1.0, -(1.0 + 2.0 ** -50)])
    R[2, 1], R[1, 2] = 1e-10, -1e-10
    assert (np.trace(R) - 1.0) / 2.0 < -1.0
    w = hc.rot2rodrigues(R)
    assert (w == 0).all() and (mr.rot2rodrigues(R) == 0).all()
    assert abs(mr.rot2rodrigues(R, fix_acos=True)[0]) > 1e5
    R = np.eye(3) * (1.0 + 2.0 ** -50)  # above +1 as well
    assert (np.trace(R) - 1.0) / 2.0 > 1.0
    assert (hc.rot2rodrigues(R) == 0).all()


def test_an_aborted_gauss_newton_leaves_x_unchanged():
    s = ms.make(ms.SEEDS[0] + 100, n=100, n_hyp=120)
    pts = hc.points(s, ms.CAM, ms.LEVEL_SIGMA2, ms.TH2)
    rp = mr.make_points(ms.CAM, s["kx"], s["ky"], s["octave"], s["world_pos"], s["slots"], ms.LEVEL_SIGMA2, ms.TH2)
    H = hc.hypotheses(pts, ms.CAM, s["sets"])
    aborted = np.flatnonzero((H["info"][:, 4] == 1) & (H["info"][:, 3] == 1))  # aborted in the first round
    assert len(aborted), "no set of this scene aborts in round 1"
    shown = 0
    for k in aborted[:5]:
        idx = s["sets"][k]
        R, t, info = mr.compute_pose(rp["f"][idx], rp["X"][idx])
        Rv, tv, _ = mr.compute_pose(rp["f"][idx], rp["X"][idx], keep_x_on_abort=False)
        if info["gap"] < 1e-9 or not info["gn"]["aborted"] or not np.isfinite(tv).all():
            continue
        assert np.abs(H["T"][k, :, :3] - R).max() < 1e-8 and np.abs(H["T"][k, :, 3] - t).max() < 1e-8
        assert np.allclose(t, info["x0"][3:], atol=0, rtol=0)  # x as the linear solution left it
        assert np.abs(H["T"][k, :, 3] - tv).max() > 1e-3       # the step that was not applied
        shown += 1
    assert shown
