"""The host build of csrc/vsg_two_view.h (tests/_twoviewcore) against the NumPy float32 restatement of
TwoViewReconstruction.cc (tests/two_view_reference.py), per hypothesis and as a whole, on the sixteen scenes of
tests/two_view_scenes.py (TUM1 intrinsics, 100 and 300 matches, general and planar, 0.5 px noise, 20 % outliers, 200 sets,
four seeds each).

The header's deviations are roundings (a double Jacobi rounded once where Eigen -- here LAPACK -- runs a float SVD; products
summed in a fixed order), so the tolerances are TWICE the largest differences measured on these scenes.  Measured (H21 and F21
scaled so that the largest entry is +1; hypotheses whose system is nearly rank deficient left out, see below):
    H21 per hypothesis 1.68e-5    F21 per hypothesis 8.20e-5    R21 2.38e-7    t21 2.12e-6    x3d 3.45e-6 (relative to |X|)
    parallax 1.7e-4 degrees (acos near 1 amplifies a float ulp of the cosine)
    recovered rotation within 0.615 degrees and translation direction within 5.86 degrees of the truth on every scene
    (the restatement: the same to three digits)
Two caps keep the comparison honest and are asserted:
    a hypothesis is left out only when its system's relative singular-value gap is below 1e-4 -- (s8 - s9) / s1 for H, s8 / s1
    for F -- and at most 5 % of a scene's hypotheses are (measured: at most 7 of 200, all of them F);
    an inlier decision is left out only within 1e-3 (relative) of its threshold, at most 1 % of the decisions (measured: 0.0092 %).
No compared decision may differ.  The planar scenes reach ReconstructH with rh_threshold = 0.40."""
import functools

import numpy as np
import pytest

import two_view_hostcore as hc
import two_view_reference as ref
import two_view_scenes as ts

F32, F64 = np.float32, np.float64
TOL = dict(H21=2 * 1.68e-5, F21=2 * 8.20e-5, R21=2 * 2.38e-7, t21=2 * 2.12e-6, x3d=2 * 3.45e-6, parallax=2 * 1.7e-4)


def scaled(M):
    M = np.asarray(M, F64).reshape(-1, 9)
    k = np.argmax(np.abs(M), 1)
    return M / M[np.arange(len(M)), k][:, None]


def rel_gap(A, model):
    s = np.linalg.svd(np.asarray(A, F64), compute_uv=False)
    return (s[7] - s[8]) / s[0] if model == 0 else s[7] / s[0]


@pytest.fixture(scope="module")
def runs():
    out = []
    for planar, n, seed, s in ts.issue_scenes():
        rh = 0.40 if planar else 0.50
        i1, i2 = ref.matches_of(s["xy1"], s["xy2"], s["matches12"])
        r = ref.reconstruct(s["xy1"], s["xy2"], s["matches12"], s["K"], s["sets"], rh_threshold=rh)
        h = hc.reconstruct(s, hc.params_blob(rh_threshold=rh))
        pn1, _ = ref.normalize(s["xy1"])
        pn2, _ = ref.normalize(s["xy2"])
        hyp = []
        for model in (0, 1):
            hh = hc.hypotheses(model, s)
            gaps = np.array([rel_gap((ref.system_h if model == 0 else ref.system_f)(pn1[i1[st]], pn2[i2[st]]), model) for st in s["sets"]])
            hyp.append((hh, (r["H"], r["F"])[model], gaps))
        out.append(dict(planar=planar, n=n, seed=seed, s=s, ref=r, hdr=h, hyp=hyp, i1=i1))
    return out


def test_hypotheses_agree_with_the_restatement(runs):
    worst = {0: 0.0, 1: 0.0}
    left_out, near, decisions = 0, 0, 0
    for run in runs:
        for model, (hh, rr, gaps) in enumerate(run["hyp"]):
            keep = gaps >= 1e-4
            assert (~keep).sum() <= 0.05 * len(keep), (run["planar"], run["n"], run["seed"], model, int((~keep).sum()))
            left_out = max(left_out, int((~keep).sum()))
            d = np.abs(scaled(hh["M21"][keep]) - scaled(rr["M21"][keep])).max()
            worst[model] = max(worst[model], d)
            # the inlier decisions of the kept hypotheses: one per match and term
            th = F32(5.991) if model == 0 else F32(3.841)
            chi = rr["chi"][keep].astype(F64)
            close = np.abs(chi - th) <= 1e-3 * th
            hdr_out = hh["terms"][keep] == 0  # a term the header did not add
            with np.errstate(invalid="ignore"):
                ref_out = chi > th
            # th - chi == 0 exactly at chi == th, which `close` covers
            assert ((hdr_out == ref_out) | close).all(), (run["planar"], run["n"], run["seed"], model)
            assert ((hh["inlier"][keep] == rr["inlier"][keep]) | close.any(2)).all()
            near += int(close.sum())
            decisions += close.size
    print("largest difference, scaled to a largest entry of +1: H21 %.2e  F21 %.2e; hypotheses left out per scene and model: at most %d "
          "of 200; decisions within 1e-3 of the threshold: %d of %d (%.4f %%)" % (worst[0], worst[1], left_out, near, decisions,
                                                                                    100.0 * near / decisions))
    assert near <= 0.01 * decisions
    assert worst[0] <= TOL["H21"] and worst[1] <= TOL["F21"]


def test_scores_select_the_same_winner_and_the_loop_transcribed_selects_the_headers(runs):
    for run in runs:
        h, r = run["hdr"], run["ref"]
        assert ref.first_maximum(h["score_h"])[0] == h["res"]["best_it_h"] == hc.first_maximum(h["score_h"])
        assert ref.first_maximum(h["score_f"])[0] == h["res"]["best_it_f"] == hc.first_maximum(h["score_f"])
        assert (h["res"]["best_it_h"], h["res"]["best_it_f"]) == (r["best_it_h"], r["best_it_f"])
        assert h["res"]["SH"] == h["score_h"][h["res"]["best_it_h"]] and h["res"]["SF"] == h["score_f"][h["res"]["best_it_f"]]
        # the sums themselves: 2 N float additions each, within N ulp of the restatement's
        assert abs(float(h["res"]["SF"]) - float(r["SF"])) <= 2e-5 * float(r["SF"])


def angle_deg(Ra, Rb):
    c = (np.trace(np.asarray(Ra, F64) @ np.asarray(Rb, F64).T) - 1) / 2
    return np.degrees(np.arccos(np.clip(c, -1, 1)))


def direction_deg(a, b):
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    return np.degrees(np.arccos(np.clip(a @ b / np.linalg.norm(a) / np.linalg.norm(b), -1, 1)))


def test_whole_routine_agrees_and_recovers_the_motion(runs):
    worst = dict(R21=0.0, t21=0.0, x3d=0.0, rot=0.0, dir=0.0, rot_ref=0.0, dir_ref=0.0, par=0.0)
    for run in runs:
        h, r, s = run["hdr"], run["ref"], run["s"]
        x = h["res"]
        tag = (run["planar"], run["n"], run["seed"])
        assert x["ok"] == 1 and r["ok"], tag
        assert x["model"] == r["model"] == (0 if run["planar"] else 1), tag
        assert x["reason"] == r["reason"] == 0 and x["n_inliers"] == r["N"], tag
        # the sign of a singular pair permutes the motion hypotheses: nGood as a multiset, the chosen one's value
        assert sorted(x["n_good"]) == sorted(list(r["n_good"]) + [0] * (8 - len(r["n_good"]))), tag
        worst["R21"] = max(worst["R21"], np.abs(x["R21"].astype(F64) - r["R"]).max())
        worst["t21"] = max(worst["t21"], np.abs(x["t21"].astype(F64) - r["t"]).max())
        worst["par"] = max(worst["par"], abs(float(x["parallax"]) - float(r["parallax"])))
        assert (h["triangulated"] == 1).tolist() == r["tri"].tolist(), tag
        if run["planar"]:
            assert (h["x3d"] == hc.X3D_SENTINEL).all(), tag  # ReconstructH never assigns vP3D
        else:
            P = r["P3D"].astype(F64)
            nz = np.linalg.norm(P, axis=1) > 0
            assert ((h["x3d"] != 0).any(1) == nz).all(), tag
            worst["x3d"] = max(worst["x3d"], (np.linalg.norm(h["x3d"][nz] - P[nz], axis=1) / np.linalg.norm(P[nz], axis=1)).max())
        worst["rot"], worst["dir"] = max(worst["rot"], angle_deg(x["R21"], s["R"])), max(worst["dir"], direction_deg(x["t21"], s["t"]))
        worst["rot_ref"] = max(worst["rot_ref"], angle_deg(r["R"], s["R"]))
        worst["dir_ref"] = max(worst["dir_ref"], direction_deg(r["t"], s["t"]))
    print("largest differences: R21 %.2e  t21 %.2e  x3d %.2e (relative)  parallax %.2e deg; recovered within %.3f deg (rotation) and "
          "%.2f deg (direction), the restatement within %.3f and %.2f" % (worst["R21"], worst["t21"], worst["x3d"], worst["par"],
                                                                         worst["rot"], worst["dir"], worst["rot_ref"], worst["dir_ref"]))
    assert worst["R21"] <= TOL["R21"] and worst["t21"] <= TOL["t21"] and worst["x3d"] <= TOL["x3d"] and worst["par"] <= TOL["parallax"]
    # 0.5 px of noise is 0.055 degrees of a ray at f = 517 px and the baseline subtends about 40 px: the rotation to a degree,
    # the direction of a translation that trades against the rotation at this field of view to ten
    assert worst["rot"] <= 1.0 and worst["dir"] <= 10.0


def selected_motions(s, params=None, sets=None):
    """The host build's call on a scene and CheckRT of every motion hypothesis of the selected model, from the call's own
    outputs: (reconstruct's dict, [check_rt's dict per motion hypothesis])."""
    h = hc.reconstruct(s, params, sets)
    res = h["res"]
    M21, inl = (res["H21"], h["inlier_h"]) if res["model"] == 0 else (res["F21"], h["inlier_f"])
    Rs, tt = hc.motions(res["model"], M21, s["K"])
    out = [hc.check_rt(R, t, s["K"], hc.matches_of(s)[1], inl) for R, t in zip(Rs, tt)]
    assert [c["n_good"] for c in out] == list(res["n_good"][:len(out)])  # the hypotheses in the call's own order
    return h, out


def rank_holder(c):
    """The first counted match whose cosine holds rank min(50, n_good - 1), and the numbers below and not above it."""
    counted = c["state"] != 0
    v, idx = c["cos"][counted], min(50, int(counted.sum()) - 1)
    for j in np.flatnonzero(counted):
        lo, le = int((v < c["cos"][j]).sum()), int((v <= c["cos"][j]).sum())
        if lo <= idx < le:
            return int(j), lo, le
    return -1, 0, 0


@functools.lru_cache(maxsize=None)
def tie_scene():
    """ts.tie_across_the_tile on the match that holds rank 50 under the chosen motion hypothesis of ts.tie_base() and the
    match of the largest cosine."""
    _, checks = selected_motions(ts.tie_base())
    c = max(checks, key=lambda c: c["n_good"])
    a = rank_holder(c)[0]
    b = int(np.argmax(np.where(c["state"] != 0, c["cos"], -2.0)))
    assert a >= 0 and a != b
    return ts.tie_across_the_tile(a, b)


@functools.lru_cache(maxsize=None)
def tile_cases():
    """name -> scene: what tests/test_gpu_two_view.py runs past the first tile of k_tv_check_rt's rank count and at the cap
    of the iterations."""
    out = {"matches_%d" % n: ts.tile_scene(n) for n in ts.TILE_SIZES}
    out["rank_holder_late"], out["tie_across_the_tile"], out["winner_last"] = ts.rank_holder_late(), tie_scene(), ts.winner_last()
    return out


@pytest.mark.parametrize("name", ["matches_%d" % n for n in ts.TILE_SIZES] + ["rank_holder_late", "tie_across_the_tile", "winner_last"])
def test_rank_count_equals_the_sort_past_the_tile(name):
    """vCosParallax[min(50, size - 1)] after std::sort, as TwoViewReconstruction.cc has it, against the header's rank count,
    for every motion hypothesis of the selected model."""
    s = tile_cases()[name]
    h, checks = selected_motions(s)
    assert len(checks) in (4, 8) and max(c["n_good"] for c in checks) > 51
    for c in checks:
        counted = c["state"] != 0
        assert int(counted.sum()) == c["n_good"]
        if c["n_good"] == 0:
            assert np.isnan(hc.ranked_cosine(c["cos"], c["state"]))
            continue
        want = np.sort(c["cos"][counted])[min(50, c["n_good"] - 1)]
        got = hc.ranked_cosine(c["cos"], c["state"])
        assert got.tobytes() == want.tobytes() == c["cosine"].tobytes(), (name, c["n_good"])


def test_tile_scene_sizes():
    for n in ts.TILE_SIZES:
        s = ts.tile_scene(n)
        assert int((s["matches12"] >= 0).sum()) == n and 0.08 * n <= s["is_outlier"].sum() <= 0.12 * n and 8 <= len(s["sets"]) <= 16
        r = hc.reconstruct(s)["res"]
        assert r["ok"] == 1 and r["model"] == 1 and max(r["n_good"]) > 0.8 * n and max(len(s["xy1"]), len(s["xy2"])) <= 4096


def test_rank_holder_lies_past_the_first_tile():
    """The directed scene: the candidate trips of the rank count pass index 1024 before a match holds rank 50."""
    s = ts.rank_holder_late()
    h, checks = selected_motions(s)
    assert int((s["matches12"] >= 0).sum()) == 1500 and h["res"]["ok"] == 1 and h["res"]["model"] == 1
    c = max(checks, key=lambda c: c["n_good"])
    j, lo, le = rank_holder(c)
    assert c["n_good"] == 1500 and j >= ts.TILE and lo <= 50 < le
    assert c["cos"][j] == hc.ranked_cosine(c["cos"], c["state"])


def test_tie_sits_across_the_tile_boundary():
    s = tie_scene()
    i1 = np.nonzero(s["matches12"] >= 0)[0]
    a, b = ts.TILE - 1, ts.TILE
    assert (s["xy1"][i1[a]] == s["xy1"][i1[b]]).all() and (s["xy2"][s["matches12"][i1[a]]] == s["xy2"][s["matches12"][i1[b]]]).all()
    assert i1[a] != i1[b] and s["matches12"][i1[a]] != s["matches12"][i1[b]] and len(i1) == 1100
    h, checks = selected_motions(s)
    c = max(checks, key=lambda c: c["n_good"])
    assert h["res"]["ok"] == 1 and c["state"][a] != 0 and c["state"][b] != 0
    v = c["cos"][c["state"] != 0]
    assert c["cos"][a].tobytes() == c["cos"][b].tobytes()
    for j in (a, b):
        assert (v < c["cos"][j]).sum() <= 50 < (v <= c["cos"][j]).sum()
    assert rank_holder(c)[0] == a and hc.ranked_cosine(c["cos"], c["state"]) == c["cos"][a]


def test_winner_last_scene_selects_the_last_iteration():
    s = ts.winner_last()
    assert len(s["sets"]) == 1024 and (s["sets"][:1023] == s["sets"][0]).all()
    assert s["is_outlier"][s["sets"][0]].all() and not s["is_outlier"][s["sets"][1023]].any()
    h = hc.reconstruct(s)
    assert h["res"]["best_it_f"] == 1023 and ref.first_maximum(h["score_f"])[0] == 1023


def test_sweep_counts_are_one_past_convergence():
    """The trial DESIGN.md records: the null vector of every system of the sixteen scenes after 1 .. 12 sweeps against
    numpy.linalg.svd in double, systems with a relative gap below 1e-4 left out."""
    A = {0: [], 1: []}
    for planar, n, seed, s in ts.issue_scenes():
        i1, i2 = ref.matches_of(s["xy1"], s["xy2"], s["matches12"])
        pn1, _ = ref.normalize(s["xy1"])
        pn2, _ = ref.normalize(s["xy2"])
        for st in s["sets"]:
            A[0].append(ref.system_h(pn1[i1[st]], pn2[i2[st]])), A[1].append(ref.system_f(pn1[i1[st]], pn2[i2[st]]))
    s9, _ = hc.sweeps()
    for model in (0, 1):
        M = np.array(A[model])
        keep = np.array([rel_gap(a, model) >= 1e-4 for a in M])
        M = M[keep]
        want = np.linalg.svd(M.astype(F64))[2][:, 8]
        errs = []
        for sw in range(1, 13):
            v = hc.null_vectors(M, sw)
            v /= np.linalg.norm(v, axis=1)[:, None]
            sign = np.sign((v * want).sum(1))[:, None]
            errs.append(np.abs(v * sign - want).max())
        print("model %d, %d systems: error after 1 .. 12 sweeps " % (model, len(M)) + " ".join("%.1e" % e for e in errs))
        final = min(errs)
        first = next(k + 1 for k, e in enumerate(errs) if e <= 10 * final)
        assert first < s9 <= first + 2, (first, s9)
