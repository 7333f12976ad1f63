"""k_stereo and the host median cut at their edges: every directed scene of tests/stereo_scenes.py (each already checked on
the CPU against the oracle and against the branch it was built for, tests/test_stereo_reference.py) through the three entry
points -- orb.ComputeStereoMatches (host arrays), orb.ComputeStereoMatches_resident and the stereo half of
orb.stereo_bow_search -- with two handles and with one handle holding the pair as a two-frame batch in either order.  Outputs
are compared with the NumPy restatement as uint32 views.  Then the launch shapes, the refusals (through the return code only)
and the window rule (stereo section)."""
import numpy as np
import pytest

import stereo_reference as sr
import stereo_scenes as ss
from visual_sgraphs_amd import orb, synth

pytestmark = pytest.mark.gpu

BOUNDS = (0.0, 0.0, float(ss.W), float(ss.H))
CONFIGS = ("two_handles", "batch_left_right", "batch_right_left")
INVALID = -6  # VSG_ERR_INVALID


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def rig():
    """Extractors (made once; each scene's images run through them again) and a small vocabulary for the fused call."""
    blob = synth.synthetic_vocabulary(6, 3, seed=31, stop_fraction=0.2)
    return dict(left=orb.ORBextractor(*ss.EXTRACTOR), right=orb.ORBextractor(*ss.EXTRACTOR),
                batch=orb.ORBextractor(*ss.EXTRACTOR, max_batch=2), voc=orb.ORBVocabulary(blob))


def pyramids_for(rig, scene, config):
    """Runs the scene's images through the extractors; returns (left handle, left frame, right handle, right frame).  The
    extractor's own keypoints are discarded: only the pyramids are used."""
    if config == "two_handles":
        rig["left"](scene["L"]), rig["right"](scene["R"])
        return rig["left"], 0, rig["right"], 0
    if config == "batch_left_right":
        rig["batch"].extract_batch(np.stack([scene["L"], scene["R"]]))
        return rig["batch"], 0, rig["batch"], 1
    rig["batch"].extract_batch(np.stack([scene["R"], scene["L"]]))
    return rig["batch"], 1, rig["batch"], 0


def frame_of(kps, desc):
    return orb.Frame(max(len(kps), 1)).upload(kps, desc, BOUNDS)


def run_three(rig, where, kl, dl, kr, dr, mb, mbf):
    """[(entry, mvuRight, mvDepth, match count or None)] of the three entry points."""
    hl, fl_i, hr, fr_i = where
    out = [("host arrays",) + tuple(orb.ComputeStereoMatches(hl, fl_i, hr, fr_i, kl, dl, kr, dr, mb, mbf)) + (None,)]
    fl, fr = frame_of(kl, dl), frame_of(kr, dr)
    out.append(("resident",) + tuple(orb.ComputeStereoMatches_resident(hl, fl_i, hr, fr_i, fl, fr, mb, mbf)) + (None,))
    got = orb.stereo_bow_search(hl, fl_i, hr, fr_i, fl, fr, mb, mbf, rig["voc"], 2)
    out.append(("stereo_bow_search", got["u_right"], got["depth"], got["n_stereo"]))
    return out


def assert_parity(results, want, tag):
    for entry, u, d, count in results:
        assert np.array_equal(bits(u), bits(want["u_right"])), (tag, entry, np.flatnonzero(bits(u) != bits(want["u_right"])))
        assert np.array_equal(bits(d), bits(want["depth"])), (tag, entry, np.flatnonzero(bits(d) != bits(want["depth"])))
        if count is not None:
            assert count == want["count"], (tag, entry)


@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("name", [s["name"] for s in ss.all_scenes()])
def test_directed_scene(rig, name, config):
    scene = next(s for s in ss.all_scenes() if s["name"] == name)
    want = ss.expected(scene)[0]
    where = pyramids_for(rig, scene, config)
    results = run_three(rig, where, scene["kl"], scene["dl"], scene["kr"], scene["dr"], scene["mb"], scene["mbf"])
    assert_parity(results, want, (name, config))


def sliced_expectation(scene, nl, nr):
    _, el, er = ss.expected(scene)
    t = el.tables()
    return sr.compute(sr.pyramids(el), sr.pyramids(er), t["scale"], t["inv_scale"], scene["kl"][:nl], scene["dl"][:nl],
                      scene["kr"][:nr], scene["dr"][:nr], scene["mb"], scene["mbf"])


@pytest.mark.parametrize("nl,nr", [(0, None), (1, None), (3, None), (4, None), (5, None),
                                   (None, 0), (None, 1), (None, 63), (None, 64), (None, 65), (None, 129)])
def test_launch_shapes(rig, nl, nr):
    """Four left keypoints per workgroup and 64 right keypoints per pass of the scan: one scene cut to each side of both."""
    scene = next(s for s in ss.all_scenes() if s["name"] == "painted_main")
    nl = len(scene["kl"]) if nl is None else nl
    nr = len(scene["kr"]) if nr is None else nr
    assert len(scene["kl"]) >= 5 and len(scene["kr"]) >= 129
    want = sliced_expectation(scene, nl, nr)
    where = pyramids_for(rig, scene, "two_handles")
    results = run_three(rig, where, scene["kl"][:nl], scene["dl"][:nl], scene["kr"][:nr], scene["dr"][:nr], scene["mb"],
                        scene["mbf"])
    assert_parity(results, want, (nl, nr))


# ------------------------------------------------------------------------------------------------------------ refusals

def refused(call):
    with pytest.raises(orb.VsgError) as e:
        call()
    return e.value.code


def test_octaves_outside_the_left_extractor_are_refused(rig):
    """A keypoint of either side with an octave outside [0, nlevels) of the left extractor: VSG_ERR_INVALID from all three
    entry points, and the next valid call is right."""
    scene = next(s for s in ss.all_scenes() if s["name"] == "painted_clamp")
    want = ss.expected(scene)[0]
    where = pyramids_for(rig, scene, "two_handles")
    hl, il, hr, ir = where
    kl, dl, kr, dr, mb, mbf = (scene[k] for k in ("kl", "dl", "kr", "dr", "mb", "mbf"))
    for side, octave in (("l", -1), ("l", ss.NLEVELS), ("r", -1), ("r", ss.NLEVELS), ("r", 1 << 20), ("l", 15)):
        bl, br = kl.copy(), kr.copy()
        (bl if side == "l" else br)["octave"][len(kl) // 2 if side == "l" else len(kr) - 1] = octave
        assert refused(lambda: orb.ComputeStereoMatches(hl, il, hr, ir, bl, dl, br, dr, mb, mbf)) == INVALID
        if 0 <= octave <= 15:  # (the resident frame itself takes octaves 0 .. 15)
            fl, fr = frame_of(bl, dl), frame_of(br, dr)
            assert refused(lambda: orb.ComputeStereoMatches_resident(hl, il, hr, ir, fl, fr, mb, mbf)) == INVALID
            assert refused(lambda: orb.stereo_bow_search(hl, il, hr, ir, fl, fr, mb, mbf, rig["voc"], 2)) == INVALID
        assert_parity(run_three(rig, where, kl, dl, kr, dr, mb, mbf), want, (side, octave))


def test_a_right_extractor_with_other_levels_is_refused(rig):
    scene = next(s for s in ss.all_scenes() if s["name"] == "painted_clamp")
    want = ss.expected(scene)[0]
    kl, dl, kr, dr, mb, mbf = (scene[k] for k in ("kl", "dl", "kr", "dr", "mb", "mbf"))
    more_levels = orb.ORBextractor(ss.NFEAT, ss.SCALE, ss.NLEVELS + 1, 20, 7)
    more_levels(scene["R"])
    narrower = orb.ORBextractor(*ss.EXTRACTOR)
    narrower(np.ascontiguousarray(scene["R"][:, :300]))
    where = pyramids_for(rig, scene, "two_handles")
    hl, il, _, _ = where
    fl, fr = frame_of(kl, dl), frame_of(kr, dr)
    for other in (more_levels, narrower):
        for a, b in ((hl, other), (other, hl)):
            assert refused(lambda: orb.ComputeStereoMatches(a, 0, b, 0, kl, dl, kr, dr, mb, mbf)) == INVALID
            assert refused(lambda: orb.ComputeStereoMatches_resident(a, 0, b, 0, fl, fr, mb, mbf)) == INVALID
            assert refused(lambda: orb.stereo_bow_search(a, 0, b, 0, fl, fr, mb, mbf, rig["voc"], 2)) == INVALID
        assert_parity(run_three(rig, where, kl, dl, kr, dr, mb, mbf), want, "after a refusal")


# --------------------------------------------------------------------------------------------------------- window rule

def test_window_rule():
    """Keypoints whose SAD windows leave their level by columns get no match and no say in the median; the others of the same
    call are the reference's.  Levels 1 and 2, left image in frame 1 of a two-frame batch (module docstring of DESIGN.md's
    stereo section: an unguarded kernel would read a neighbouring row of the same allocation, so a wrong rule shows as a
    wrong value)."""
    scene = ss.guard_scene()
    want = ss.expected(scene, True)[0]
    off = want["reason"] == sr.WINDOW
    assert off.sum() >= 8 and (want["u_right"][~off] >= 0).any()
    ex = orb.ORBextractor(*ss.EXTRACTOR, max_batch=2)
    ex.extract_batch(np.stack([scene["R"], scene["L"]]))
    blob = synth.synthetic_vocabulary(6, 3, seed=31, stop_fraction=0.2)
    rig = dict(voc=orb.ORBVocabulary(blob))
    results = run_three(rig, (ex, 1, ex, 0), scene["kl"], scene["dl"], scene["kr"], scene["dr"], scene["mb"], scene["mbf"])
    assert_parity(results, want, "window rule")
    for _, u, d, _ in results:
        assert (u[off] == -1).all() and (d[off] == -1).all()
