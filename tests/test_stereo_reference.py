"""The restatement of Frame::ComputeStereoMatches (tests/stereo_reference.py) against the oracle on every directed scene of
tests/stereo_scenes.py, and every directed case against the branch it was built for.  CPU only: the conditions here are on the
scenes and on the restatement, so that tests/test_gpu_stereo_edges.py compares the device with something already known to take
every branch.

Two things the scenes can NOT show, with the reasons:

  * reason DELTA_R never occurs.  bestincR is the FIRST minimum of the 11 SADs and is not at an end, so dist1 > dist2 and
    dist3 >= dist2; then |dist1 - dist3| <= max(dist1, dist3) - dist2 <= dist1 + dist3 - 2 dist2, and |deltaR| <= 0.5.  The
    test asserts that no scene produces it.
  * `bestuR = uL - 0.01` in double and `uL - 0.01f` in float give the same float for every uL whose windows lie inside the
    image.  The two differ only where the rounding boundary of the result falls between uL - 0.01 and uL - 0.01f (2.2e-10
    apart): for float32 uL that is 0.04125 <= uL <= 0.0725, and a keypoint there has no 11 x 11 window in the image.
    test_double_and_float_clamp_agree_on_every_coordinate_inside_the_image walks every float32 of [9, 320) to show it; the
    clamp cases are asserted against the double form."""
import numpy as np
import pytest

import oracle_lib as ol
import stereo_reference as sr
import stereo_scenes as ss

F32 = np.float32
PRE_SAD = (sr.NO_CANDIDATE, sr.OCTAVE_GATE, sr.U_WINDOW, sr.HAMMING_HIGH, sr.BEST_HAMMING, sr.ENDU, sr.WINDOW)


def scene_names():
    return [s["name"] for s in ss.all_scenes()]


def by_name(name):
    return next(s for s in ss.all_scenes() if s["name"] == name)


def bits(a):
    return np.asarray(a, F32).view(np.uint32)


def check_case(scene, res, i, check, arg):
    """One directed case against the restatement's result.  A miss is an error in the scene."""
    why, tag = int(res["reason"][i]), (scene["name"], i, check, arg, sr.REASON_NAMES[int(res["reason"][i])])
    if check == "reason":
        assert why == arg, tag
    elif check == "matched":  # ... with the right keypoint `arg`
        assert why == sr.MATCHED and res["best_idx"][i] == arg, tag
    elif check == "winner":
        assert res["best_idx"][i] == arg, tag
    elif check == "not_winner":
        assert res["best_idx"][i] != arg, tag
    elif check == "tie":  # two candidates at the minimum Hamming distance, the first of them wins and shows in the output
        assert res["n_at_min"][i] >= 2 and res["best_idx"][i] == arg and res["last_at_min"][i] != arg, tag
        assert why == sr.MATCHED and abs(int(res["best_inc"][i])) == 3, tag
    elif check == "sad_tie":
        first, zeros = arg
        prof = res["profile"][i]
        at_min = [k - sr.L for k in np.flatnonzero(prof == prof.min())]
        assert at_min == zeros and len(zeros) >= 2 and res["best_inc"][i] == first != zeros[-1], tag + (at_min,)
        assert why == (sr.SHIFT_EDGE if first == -sr.L else sr.MATCHED), tag
    elif check == "shift":
        assert why == sr.MATCHED and res["best_inc"][i] == arg, tag
    elif check == "clamp":
        ul, prof, k = F32(scene["kl"]["x"][i]), res["profile"][i], sr.L + int(res["best_inc"][i])
        assert why == sr.CLAMPED and res["clamped"][i] and res["best_inc"][i] == 0 and prof[k - 1] == prof[k + 1], tag
        assert bits(res["u_right"][i]) == bits(F32(np.float64(ul) - 0.01)), tag
        assert bits(res["depth"][i]) == bits(F32(F32(scene["mbf"]) / F32(0.01))), tag
    elif check in ("sad_cut", "sad_kept"):
        assert res["sad"][i] == arg and why == (sr.MEDIAN_CUT if check == "sad_cut" else sr.MATCHED), tag
    elif check == "kept":
        assert why in (sr.MATCHED, sr.MEDIAN_CUT), tag
    elif check == "searched":  # the SAD search ran
        assert why not in PRE_SAD and res["profile"][i].min() >= 0, tag
    elif check == "window":
        assert why == sr.WINDOW, tag
    else:
        raise AssertionError(check)


@pytest.mark.parametrize("name", scene_names())
def test_restatement_is_the_oracle_bit_for_bit(name):
    scene = by_name(name)
    res, el, er = ss.expected(scene)
    want_u, want_d = ol.stereo_matches(el, er, scene["kl"], scene["dl"], scene["kr"], scene["dr"], scene["mb"], scene["mbf"])
    assert np.array_equal(bits(res["u_right"]), bits(want_u))
    assert np.array_equal(bits(res["depth"]), bits(want_d))
    assert res["count"] == int(((res["reason"] == sr.MATCHED) | (res["reason"] == sr.CLAMPED)).sum())


@pytest.mark.parametrize("name", scene_names())
def test_every_directed_case_lands_on_its_branch(name):
    scene = by_name(name)
    res, _, _ = ss.expected(scene)
    for i, check, arg in scene["cases"]:
        check_case(scene, res, i, check, arg)


def test_every_reason_occurs():
    seen = np.zeros(13, np.int64)
    for scene in ss.all_scenes():
        seen += np.bincount(ss.expected(scene)[0]["reason"], minlength=13)
    for why in sr.REFERENCE_REASONS:
        if why == sr.DELTA_R:
            assert seen[why] == 0  # unreachable: module docstring
        else:
            assert seen[why] > 0, sr.REASON_NAMES[why]
    assert seen[sr.WINDOW] == 0  # parity scenes never meet the device's window rule


def test_scenes_stay_inside_the_image():
    """No SAD window of a parity scene leaves its level (the oracle's border is never read), and with the device's window rule
    the restatement gives the same bits."""
    for scene in ss.all_scenes():
        plain, guarded = ss.expected(scene)[0], ss.expected(scene, True)[0]
        assert np.array_equal(plain["reason"], guarded["reason"]), scene["name"]
        assert np.array_equal(bits(plain["u_right"]), bits(guarded["u_right"]))
        assert np.array_equal(bits(plain["depth"]), bits(guarded["depth"]))


def test_double_and_float_clamp_agree_on_every_coordinate_inside_the_image():
    lo, hi = F32(9.0).view(np.uint32), F32(ss.W).view(np.uint32)
    for a in range(int(lo), int(hi), 1 << 22):
        ul = np.arange(a, min(a + (1 << 22), int(hi)), dtype=np.uint32).view(F32)
        assert np.array_equal((ul.astype(np.float64) - 0.01).astype(F32), ul - F32(0.01))
    ul = np.arange(F32(0.04).view(np.uint32), F32(0.08).view(np.uint32), dtype=np.uint32).view(F32)
    differ = ul[(ul.astype(np.float64) - 0.01).astype(F32) != ul - F32(0.01)]  # ... and where they do differ no window fits
    assert len(differ) and 0.04 < differ.min() and differ.max() < 0.08


def test_roundf_is_half_away_from_zero():
    assert [float(sr.roundf(v)) for v in (0.5, 1.5, 2.5, 160.5, -0.5, -2.5, 0.49999997)] == [1, 2, 3, 161, -1, -3, 0]
    scene = by_name("painted_clamp")
    halves = [i for i in range(len(scene["kl"])) if scene["kl"]["x"][i] % 1 == 0.5 or scene["kl"]["y"][i] % 1 == 0.5]
    halves_r = [j for j in range(len(scene["kr"])) if scene["kr"]["x"][j] % 1 == 0.5]
    assert len(halves) >= 2 and len(halves_r) >= 2
    for k, f in ((scene["kl"][halves], "x"), (scene["kl"][halves], "y"), (scene["kr"][halves_r], "x")):
        v = k[f][k[f] % 1 == 0.5]
        assert len(v) and (np.floor(v) % 2 == 0).all()  # round-half-even would go DOWN on each of them


def test_guard_scene_on_the_cpu():
    """The window rule's scene: without the rule the restatement is still the oracle (which reads its border); with it the
    directed keypoints, and only they, get no match."""
    scene = ss.guard_scene()
    plain, el, er = ss.expected(scene)
    want_u, want_d = ol.stereo_matches(el, er, scene["kl"], scene["dl"], scene["kr"], scene["dr"], scene["mb"], scene["mbf"])
    assert np.array_equal(bits(plain["u_right"]), bits(want_u)) and np.array_equal(bits(plain["depth"]), bits(want_d))
    guarded = ss.expected(scene, True)[0]
    for i, check, arg in scene["cases"]:
        check_case(scene, guarded, i, check, arg)
        assert plain["reason"][i] not in PRE_SAD  # the reference searched every one of them
    assert (guarded["u_right"][guarded["reason"] == sr.WINDOW] == -1).all()
    off = guarded["reason"] == sr.WINDOW
    assert (plain["u_right"][off] >= 0).any() and (guarded["u_right"][~off] >= 0).any()


def test_only_candidate_below_75_at_index_64():
    """nR = 65: the second pass of the device's scan holds the winner alone."""
    scene = by_name("painted_nr65")
    want = ss.expected(scene)[0]
    assert len(scene["kr"]) == 65 and want["best_idx"][0] == 64 and want["reason"][0] == sr.MATCHED
    assert (sr.hamming(scene["dl"][0], scene["dr"][:64]) >= sr.TH_ORB).all()
    assert (sr.hamming(scene["dl"][0], scene["dr"][:64]) < sr.TH_HIGH).all()  # ... and every one of them is a candidate
