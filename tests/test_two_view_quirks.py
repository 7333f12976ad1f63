"""The quirks of TwoViewReconstruction.cc that csrc/vsg_two_view.h keeps, each pinned on the host build against the
restatement as the reference has it AND against a restatement that "fixes" the quirk: the header must side with the former
and differ from the latter."""
import numpy as np

import two_view_hostcore as hc
import two_view_reference as ref
import two_view_scenes as ts
from test_two_view_reference import TOL, scaled

F32, F64, U8 = np.float32, np.float64, np.uint8


def test_normalize_runs_over_all_keypoints_not_the_matched_ones():
    s = ts.issue_scene(11, 100, False)  # 37 and 53 unmatched keypoints interleaved
    i1, i2 = ref.matches_of(s["xy1"], s["xy2"], s["matches12"])
    nm, T = hc.normalize(s["xy1"])
    _, T_all = ref.normalize(s["xy1"])
    _, T_matched = ref.normalize(s["xy1"], over=s["xy1"][i1])
    assert np.abs(T - T_all).max() <= 1e-6 * np.abs(T_all).max()
    assert np.abs(T - T_matched).max() > 1e-3 * np.abs(T_all).max()
    sets = s["sets"][:20]
    got = scaled(hc.hypotheses(1, s, sets)["M21"])
    kept = scaled(ref.find(1, s["xy1"], s["xy2"], i1, i2, sets, 1.0)["M21"])
    fixed = scaled(ref.find(1, s["xy1"], s["xy2"], i1, i2, sets, 1.0, normalize_over_matches=True)["M21"])
    # the eight-point solution depends on the normalisation at the level of the noise, far above the rounding
    assert np.median(np.abs(got - kept).max(1)) <= TOL["F21"] < np.median(np.abs(got - fixed).max(1))


def test_fundamental_gates_at_3_841_and_scores_against_5_991():
    s = ts.issue_scene(12, 300, False)
    h = hc.reconstruct(s)
    m = hc.matches_of(s)[1][:, :4]
    F21 = h["res"]["F21"]
    kept = ref.check_fundamental(F21, m, 1.0)
    same_threshold = ref.check_fundamental(F21, m, 1.0, th=3.841, th_score=3.841)
    wide_gate = ref.check_fundamental(F21, m, 1.0, th=5.991, th_score=5.991)
    SF = float(h["res"]["SF"])
    assert abs(SF - float(kept[0])) <= 2e-5 * SF
    assert abs(SF - float(same_threshold[0])) > 0.2 * SF and abs(SF - float(wide_gate[0])) > 1e-3 * SF
    assert h["inlier_f"].astype(bool).tolist() == kept[1].tolist() != wide_gate[1].tolist()
    # a term in (3.841, 5.991] is gated out although it would still score
    chi = kept[3]
    assert ((chi > F32(3.841)) & (chi <= F32(5.991))).any()


def test_strict_first_maximum():
    nan = np.nan
    cases = [([1, 3, 3, 2], 1), ([0, 0, 0], -1), ([nan, 2, nan, 2], 1), ([nan, nan], -1), ([5], 0), ([-1, 0, 1e-30], 2),
             ([2, nan, 3, 3, nan], 2), ([np.inf, np.inf], 0)]
    for scores, want in cases:
        assert hc.first_maximum(scores) == want == ref.first_maximum(np.array(scores, F32))[0], scores
    # the restatement with >= would take the LAST of equal maxima
    last = max(k for k, v in enumerate([1, 3, 3, 2]) if v == 3)
    assert hc.first_maximum([1, 3, 3, 2]) != last


def test_low_parallax_points_count_and_are_written_but_are_not_flagged():
    s = ts.make(61, n=60, outliers=0.0, noise=0.0, deg=0.0, t=(-0.001, 0.0, 0.0), n_iter=8)  # 1 mm before points 3-8 m away
    _, m = hc.matches_of(s)
    R, t = np.eye(3, dtype=F32), np.array([-1, 0, 0], F32)
    got = hc.check_rt(R, t, s["K"], m, np.ones(len(m), U8))
    i1 = np.nonzero(s["matches12"] >= 0)[0]
    kept = ref.check_rt(R, t, m[:, :4], i1, np.ones(len(m), bool), s["K"], len(s["xy1"]), F32(4.0))
    fixed = ref.check_rt(R, t, m[:, :4], i1, np.ones(len(m), bool), s["K"], len(s["xy1"]), F32(4.0), flag_all_counted=True)
    assert got["n_good"] == kept[0] == fixed[0] == len(m)
    assert (got["state"] == 1).all() and not kept[2].any() and fixed[2].sum() == len(m)  # counted, none flagged
    assert (np.abs(got["pos"]) > 0).any(1).all()                                          # and every position written
    # the whole routine: such a pair never initialises, whichever hypothesis
    assert hc.reconstruct(s)["res"]["ok"] == 0


def test_parallax_is_the_element_min_50_size_minus_1_of_the_ascending_cosines():
    rng = np.random.default_rng(7)
    for size in (1, 2, 50, 51, 52, 53, 200):
        cosv = rng.uniform(0.9, 1.0, size + 30).astype(F32)
        cosv[rng.integers(0, len(cosv), 10)] = cosv[0]  # ties
        state = np.ones(len(cosv), U8)
        state[rng.choice(len(cosv), 30, replace=False)] = 0  # not counted: never read
        cosv[state == 0] = -5.0
        counted = np.sort(cosv[state != 0])
        assert len(counted) == size
        got = hc.ranked_cosine(cosv, state)
        assert got == counted[min(50, size - 1)], size
        if size >= 53:
            assert got != counted[size // 2] and got != counted[-1]  # neither the median nor the last
    assert np.isnan(hc.ranked_cosine(np.zeros(4, F32), np.zeros(4, U8)))


def test_reconstruct_h_never_assigns_the_points_and_f_assigns_them_whole():
    rng = np.random.default_rng(5)
    s = ts.issue_scene(12, 100, True)
    before = rng.normal(size=(len(s["xy1"]), 3)).astype(F32)
    h = hc.reconstruct(s, hc.params_blob(rh_threshold=0.40), x3d_init=before)
    assert h["res"]["ok"] == 1 and h["res"]["model"] == 0
    assert h["x3d"].tobytes() == before.tobytes()                      # vP3D as the caller left it (:724-730)
    assert set(np.unique(h["triangulated"])) == {0, 1}                 # vbTriangulated IS assigned (:727)
    g = ts.issue_scene(11, 100, False)
    before = rng.normal(size=(len(g["xy1"]), 3)).astype(F32)
    f = hc.reconstruct(g, x3d_init=before)
    assert f["res"]["ok"] == 1 and f["res"]["model"] == 1
    written = (f["x3d"] != 0).any(1)
    assert written.sum() == max(f["res"]["n_good"]) and (f["x3d"][~written] == 0).all()  # whole: zero where CheckRT wrote nothing
    assert (f["triangulated"][~written] == 0).all()
    # a failed call assigns neither
    bad = hc.reconstruct(g, hc.params_blob(rh_threshold=0.0), x3d_init=before)
    assert bad["res"]["ok"] == 0 and bad["x3d"].tobytes() == before.tobytes() and (bad["triangulated"] == 0xAA).all()
