"""SearchForTriangulation with the epipole gate and Pinhole::epipolarConstrain on the device
(vsg_frame_search_for_triangulation_epipolar, k_triangulation_walk<EpipolarPred>) on the parity scene of tests/epipolar_scenes.py: the
restatement's bitmask (tests/epipolar_reference.py) goes into the EXISTING CPU oracle of the triangulation search, and the new
call -- and the existing resident call fed the same bits -- must return the oracle's matches12 and count.  The device
predicate is compared pair by pair through vsg_debug_epipolar_pairs, on the scene's largest node and on the directed edge
cases of the CPU test.  Then the resident FeatureVectors, and the arguments the call must refuse before it enqueues."""
import numpy as np
import pytest

import epipolar_reference as er
import epipolar_scenes as es
import oracle_lib as ol
from visual_sgraphs_amd import orb, synth

pytestmark = pytest.mark.gpu
F32 = np.float32
INVALID, UNSUPPORTED = -6, -3


@pytest.fixture(scope="module")
def scene():
    s = dict(es.frames())
    er.check_scene([es.leg_scene(s, leg) for leg in es.LEGS])
    cap = max(len(s["k1"]), len(s["k2"])) + 1
    s["F1"] = orb.Frame(cap).upload(s["k1"], s["d1"], es.BOUNDS, u_right=s["ur1"])
    s["F2"] = orb.Frame(cap).upload(s["k2"], s["d2"], es.BOUNDS, u_right=s["ur2"])
    s["F1_mono"] = orb.Frame(cap).upload(s["k1"], s["d1"], es.BOUNDS)
    s["F2_mono"] = orb.Frame(cap).upload(s["k2"], s["d2"], es.BOUNDS)
    return s


def expected(s, ref, ori, fv1=None, fv2=None):
    """The existing CPU oracle fed the restatement's bits."""
    return ol.search_for_triangulation(s["d1"], s["k1"]["angle"], ref["eligible1"], fv1 or s["fv1"], s["d2"], s["k2"]["angle"],
                                       ref["eligible2"], fv2 or s["fv2"], ref["pair_ok"], ref["pair_off"], ori)


def run(s, leg, ori, no_mp1=None, no_mp2=None, fv=True):
    key, only_stereo, coarse, u1, u2 = es.LEGS[leg]
    f1, f2 = s["F1" if u1 else "F1_mono"], s["F2" if u2 else "F2_mono"]
    m1 = s["no_mp1"] if no_mp1 is None else no_mp1
    m2 = s["no_mp2"] if no_mp2 is None else no_mp2
    return f1.SearchForTriangulationEpipolar(m1, f2, m2, s[key], s["ep"], s["sf"], s["sigma2"], only_stereo, coarse, ori,
                                             s["fv1"] if fv else None, s["fv2"] if fv else None)


@pytest.mark.parametrize("ori", [True, False], ids=["orientation", "no_orientation"])
@pytest.mark.parametrize("leg", list(es.LEGS))
def test_matches_equal_the_oracle_fed_the_restatement_bits(scene, leg, ori):
    s = scene
    ref = es.leg_scene(s, leg)
    want = expected(s, ref, ori)
    got = run(s, leg, ori)
    assert got[0] == want[0] and np.array_equal(got[1], want[1])
    # the existing resident search with the same bits agrees too
    key, only_stereo, coarse, u1, u2 = es.LEGS[leg]
    old = s["F1"].SearchForTriangulation(ref["eligible1"], s["fv1"], s["F2"], ref["eligible2"], s["fv2"], ori, ref["pair_ok"],
                                         ref["pair_off"])
    assert old[0] == want[0] and np.array_equal(old[1], want[1])
    if leg in ("plain", "coarse", "kf1_without_uright"):
        assert want[0] >= 40
    if leg == "plain" and not ori:
        # the later of two equal candidates wins: some matched partner has a twin (same descriptor and keypoint) EARLIER in
        # its node's KF2 list, which a first-wins scan would have returned instead
        ids2, off2, idx2 = s["fv2"]
        later = 0
        for j in want[1][want[1] >= 0]:
            at = int(np.flatnonzero(idx2 == j)[0])
            b = int(np.searchsorted(off2, at, side="right")) - 1
            before = idx2[off2[b]:at]
            later += bool(len(before) and ((s["d2"][before] == s["d2"][j]).all(1) & (s["k2"][before] == s["k2"][j])).any())
        assert later >= 1


def test_every_flag_zero_on_one_side_and_an_empty_frame(scene):
    s = scene
    n1, n2 = len(s["k1"]), len(s["k2"])
    for m1, m2 in ((np.zeros(n1, np.uint8), None), (None, np.zeros(n2, np.uint8))):
        ref = es.leg_scene(s, "plain", m1, m2)
        want = expected(s, ref, True)
        got = run(s, "plain", True, m1, m2)
        assert want[0] == 0 and got[0] == 0 and (got[1] == -1).all()
    empty = orb.Frame(4).upload(s["k1"][:0], s["d1"][:0], es.BOUNDS)
    none = (np.zeros(0, np.int32), np.zeros(1, np.int32), np.zeros(0, np.int32))
    args = (s["F12"], s["ep"], s["sf"], s["sigma2"], False, False, True)
    nm, m = empty.SearchForTriangulationEpipolar(np.zeros(0, np.uint8), s["F2"], s["no_mp2"], *args, none, s["fv2"])
    assert nm == 0 and len(m) == 0
    nm, m = s["F1"].SearchForTriangulationEpipolar(s["no_mp1"], empty, np.zeros(0, np.uint8), *args, s["fv1"], none)
    assert nm == 0 and len(m) == n1 and (m == -1).all()
    # NULL FeatureVectors: an empty frame has an empty FeatureVector whatever ComputeBoW left
    nm, m = s["F1"].SearchForTriangulationEpipolar(s["no_mp1"], empty, np.zeros(0, np.uint8), *args)
    assert nm == 0 and (m == -1).all()


@pytest.mark.parametrize("leg", list(es.LEGS))
def test_device_reasons_equal_the_restatement_on_the_largest_node(scene, leg):
    s = scene
    key, only_stereo, coarse, u1, u2 = es.LEGS[leg]
    ref = es.leg_scene(s, leg)
    big = np.bincount(ref["node"]).argmax()
    sel = ref["node"] == big
    assert sel.sum() > es.TILE * es.TILE
    got = orb.debug_epipolar_pairs(s["F1" if u1 else "F1_mono"], s["F2" if u2 else "F2_mono"], ref["i1"][sel], ref["i2"][sel],
                                   s[key], s["ep"], s["sf"], s["sigma2"], only_stereo, coarse)
    assert np.array_equal(got, ref["reason"][sel])


def test_device_reasons_equal_the_restatement_on_the_directed_cases():
    sf = (F32(1.2) ** np.arange(8, dtype=F32)).astype(F32)
    sigma2 = (sf * sf).astype(F32)
    cases = es.directed_cases(sf, sigma2)
    assert len(cases) >= 25
    seen = set()
    for name, c in cases.items():
        n = len(c["x2"])
        k1, k2 = np.zeros(n, orb.KP_DTYPE), np.zeros(n, orb.KP_DTYPE)
        k1["x"], k1["y"], k2["x"], k2["y"], k2["octave"] = c["x1"], c["y1"], c["x2"], c["y2"], c["octave2"]
        d = np.zeros((n, 32), np.uint8)
        f1 = orb.Frame(n).upload(k1, d, (0.0, 0.0, 640.0, 480.0), u_right=c["ur1"])
        f2 = orb.Frame(n).upload(k2, d, (0.0, 0.0, 640.0, 480.0), u_right=c["ur2"])
        got = orb.debug_epipolar_pairs(f1, f2, np.arange(n), np.arange(n), c["F12"], c["ep"], sf, sigma2, c["only_stereo"],
                                       c["coarse"])
        assert np.array_equal(got, c["reason"]), name
        seen |= set(got.tolist())
        f1.close(), f2.close()
    assert seen == {er.PASS, er.NOT_STEREO, er.EPIPOLE_GATE, er.DEN_ZERO, er.CHI_SQUARE}


def test_resident_feature_vectors_and_a_frame_without_compute_bow(scene):
    """The k = 10 / L = 6 vocabulary of tests/test_gpu_bow_resident.py: the NULL-FeatureVector call equals the
    host-FeatureVector call given the FeatureVectors read back (and the oracle); a frame that never had its ComputeBoW is
    VSG_ERR_INVALID, and the next call on this thread is right again."""
    s = scene
    voc = orb.ORBVocabulary(synth.synthetic_vocabulary(10, 6, seed=17, stop_fraction=0.05))
    cap = max(len(s["k1"]), len(s["k2"])) + 1
    f1 = orb.Frame(cap).upload(s["k1"], s["d1"], es.BOUNDS, u_right=s["ur1"])
    f2 = orb.Frame(cap).upload(s["k2"], s["d2"], es.BOUNDS, u_right=s["ur2"])
    args = (s["F12"], s["ep"], s["sf"], s["sigma2"], False, False, True)
    fv1 = f1.ComputeBoW(voc)["fv"]
    with pytest.raises(orb.VsgError) as e:
        f1.SearchForTriangulationEpipolar(s["no_mp1"], f2, s["no_mp2"], *args)
    assert e.value.code == INVALID
    fv2 = f2.ComputeBoW(voc)["fv"]
    assert len(np.intersect1d(fv1[0], fv2[0])) >= 20
    res = f1.SearchForTriangulationEpipolar(s["no_mp1"], f2, s["no_mp2"], *args)
    host = f1.SearchForTriangulationEpipolar(s["no_mp1"], f2, s["no_mp2"], *args, fv1, fv2)
    ref = er.scene(s["k1"], s["ur1"], s["no_mp1"], fv1, s["d1"], s["k2"], s["ur2"], s["no_mp2"], fv2, s["d2"], s["F12"], s["ep"],
                   s["sf"], s["sigma2"], False, False)
    want = expected(s, ref, True, fv1, fv2)
    assert want[0] >= 20
    assert res[0] == host[0] == want[0] and np.array_equal(res[1], want[1]) and np.array_equal(host[1], want[1])
    # an upload makes the FeatureVector stale again
    f2.upload(s["k2"], s["d2"], es.BOUNDS, u_right=s["ur2"])
    with pytest.raises(orb.VsgError) as e:
        f1.SearchForTriangulationEpipolar(s["no_mp1"], f2, s["no_mp2"], *args)
    assert e.value.code == INVALID
    again = f1.SearchForTriangulationEpipolar(s["no_mp1"], f2, s["no_mp2"], *args, fv1, fv2)
    assert again[0] == want[0] and np.array_equal(again[1], want[1])


def test_bad_arguments_are_refused_before_anything_is_enqueued(scene):
    """Through the return code only; a valid call afterwards is right."""
    s = scene
    n1, n2 = len(s["k1"]), len(s["k2"])
    args = (s["F12"], s["ep"], s["sf"], s["sigma2"], False, False, True)

    def code(f1, m1, f2, m2, *a):
        with pytest.raises(orb.VsgError) as e:
            f1.SearchForTriangulationEpipolar(m1, f2, m2, *a)
        return e.value.code

    ids, off, idx = s["fv1"]
    for bad in (n1, -1, 1 << 30):          # an idx outside [0, n)
        bidx = idx.copy()
        bidx[len(bidx) // 2] = bad
        assert code(s["F1"], s["no_mp1"], s["F2"], s["no_mp2"], *args, (ids, off, bidx), s["fv2"]) == INVALID
    ids2, off2, idx2 = s["fv2"]
    bidx = idx2.copy()
    bidx[-1] = n2
    assert code(s["F1"], s["no_mp1"], s["F2"], s["no_mp2"], *args, s["fv1"], (ids2, off2, bidx)) == INVALID
    boff = off.copy()
    boff[2] = boff[3] + 1                  # offsets that do not ascend
    assert code(s["F1"], s["no_mp1"], s["F2"], s["no_mp2"], *args, (ids, boff, idx), s["fv2"]) == INVALID
    top = int(s["k2"]["octave"].max())     # an octave of KF2 >= nlevels
    assert top >= 1
    short = (s["F12"], s["ep"], s["sf"][:top], s["sigma2"][:top], False, False, True)
    assert code(s["F1"], s["no_mp1"], s["F2"], s["no_mp2"], *short, s["fv1"], s["fv2"]) == INVALID
    seventeen = (s["F12"], s["ep"], np.ones(17, F32), np.ones(17, F32), False, False, True)
    assert code(s["F1"], s["no_mp1"], s["F2"], s["no_mp2"], *seventeen, s["fv1"], s["fv2"]) == INVALID
    rig = orb.Frame(n2 + 1).upload(s["k2"], s["d2"], es.BOUNDS, nleft=n2 // 2)   # Nleft != -1
    assert code(s["F1"], s["no_mp1"], rig, s["no_mp2"], *args, s["fv1"], s["fv2"]) == UNSUPPORTED
    rig1 = orb.Frame(n1 + 1).upload(s["k1"], s["d1"], es.BOUNDS, nleft=n1 // 2)
    assert code(rig1, s["no_mp1"], s["F2"], s["no_mp2"], *args, s["fv1"], s["fv2"]) == UNSUPPORTED
    if orb.device_count() > 1:             # frames on different devices
        other = orb.Frame(n2 + 1, device=1).upload(s["k2"], s["d2"], es.BOUNDS, u_right=s["ur2"])
        assert code(s["F1"], s["no_mp1"], other, s["no_mp2"], *args, s["fv1"], s["fv2"]) == INVALID
    with pytest.raises(orb.VsgError) as e:  # the hook checks its pairs the same way
        orb.debug_epipolar_pairs(s["F1"], s["F2"], [0, n1], [0, 0], s["F12"], s["ep"], s["sf"], s["sigma2"], False, False)
    assert e.value.code == INVALID
    ref = es.leg_scene(s, "plain")
    want = expected(s, ref, True)
    got = run(s, "plain", True)
    assert got[0] == want[0] > 0 and np.array_equal(got[1], want[1])
