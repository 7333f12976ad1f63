"""GPU parity of the DBoW2 vocabulary transform and the C3 chain
extract -> ComputeBoW -> SearchByBoW with a synthetic vocabulary (the real ORBvoc.txt.bin is a missing blob)."""
import numpy as np
import pytest

import oracle_lib as ol
from visual_sgraphs_amd import orb, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def frames():
    e = ol.OracleExtractor(1200, 1.2, 8, 20, 7)
    _, k0, d0 = e(synth.sequence_frame(752, 480, 13, 0))
    _, k1, d1 = e(synth.sequence_frame(752, 480, 13, 1))
    return (k0, d0), (k1, d1)


# (10, 6, levelsup 4) is the reference's scale: ORBvoc.txt.bin is k = 10, L = 6 (1 111 111 nodes, 10^6 words) and
# Frame::ComputeBoW / KeyFrame::ComputeBoW call transform(..., 4) (Frame.cc:887, KeyFrame.cc:106), which puts the
# FeatureVector nodes at level 2 = ~100 nodes.  The 50 MB vocabulary image is generated on the fly, never committed.
@pytest.mark.parametrize("k,L,levelsup,scoring,weighting", [(10, 3, 2, 0, 0), (10, 4, 4, 0, 0), (8, 3, 1, 1, 1),
                                                            (10, 3, 5, 5, 0), (6, 4, 2, 2, 2), (10, 3, 2, 0, 3),
                                                            (10, 6, 4, 0, 0)])
def test_bow_transform_matches_dbow2_restatement(frames, k, L, levelsup, scoring, weighting):
    (k0, d0), _ = frames
    blob = synth.synthetic_vocabulary(k, L, seed=k * 10 + L, scoring=scoring, weighting=weighting)
    ref, voc = ol.OracleVocabulary(blob), orb.ORBVocabulary(blob)
    assert (voc.k, voc.L, voc.scoring, voc.weighting, voc.nnodes, voc.nwords) == \
        (ref.k, ref.L, ref.scoring, ref.weighting, ref.nnodes, ref.nwords)
    want, got = ref.transform(d0, levelsup), voc.transform(d0, levelsup)
    for key in ("word", "node", "bow_ids"):
        assert np.array_equal(got[key], want[key]), key
    assert np.array_equal(got["weight"].view(np.uint64), want["weight"].view(np.uint64))
    assert np.array_equal(got["bow_vals"].view(np.uint64), want["bow_vals"].view(np.uint64))  # bit-identical doubles
    for a, b in zip(got["fv"], want["fv"]):
        assert np.array_equal(a, b)
    assert len(want["bow_ids"]) > 20


def test_bow_transform_ties_take_first_child():
    """All-equal node descriptors: every distance ties, the first child must win at every level."""
    import struct
    k, L = 4, 3
    n_nodes = (k ** (L + 1) - 1) // (k - 1)
    first_leaf = (k ** L - 1) // (k - 1)
    blob = bytearray(struct.pack("<iiii", k, L, 0, 0))
    for i in range(1, n_nodes):
        blob += struct.pack("<iB", (i - 1) // k, 1 if i >= first_leaf else 0) + bytes(32) + struct.pack("<d", 1.0)
    desc = synth.random_descriptors(50, 3)
    ref, voc = ol.OracleVocabulary(bytes(blob)), orb.ORBVocabulary(bytes(blob))
    want, got = ref.transform(desc, 1), voc.transform(desc, 1)
    assert np.array_equal(got["word"], want["word"]) and np.all(want["word"] == 0)
    assert np.array_equal(got["node"], want["node"])


@pytest.fixture(scope="module")
def reference_scale_vocabulary():
    blob = synth.synthetic_vocabulary(10, 6, seed=7)
    return ol.OracleVocabulary(blob), orb.ORBVocabulary(blob)


def test_reference_scale_vocabulary_shapes(frames, reference_scale_vocabulary):
    """k = 10, L = 6, levelsup = 4: the FeatureVector has on the order of 100 level-2 nodes with ~10 features each --
    the shape SearchByBoW sees in the reference (with L <= 4 and levelsup 4 it collapses to one node)."""
    ref, voc = reference_scale_vocabulary
    assert (voc.k, voc.L, voc.nnodes, voc.nwords) == (10, 6, 1111111, 1000000) == (ref.k, ref.L, ref.nnodes, ref.nwords)
    (k0, d0), _ = frames
    got, want = voc.transform(d0, 4), ref.transform(d0, 4)
    assert 60 <= len(want["fv"][0]) <= 100 and np.all(want["fv"][0] >= 11) and np.all(want["fv"][0] <= 110)
    for a, b in zip(got["fv"], want["fv"]):
        assert np.array_equal(a, b)
    assert np.array_equal(got["bow_ids"], want["bow_ids"])
    assert np.array_equal(got["bow_vals"].view(np.uint64), want["bow_vals"].view(np.uint64))


def test_c3_chain_at_reference_vocabulary_scale(reference_scale_vocabulary):
    """Config C3 as BASELINE.json states it, every step on device-resident data: stereo pair -> two extractors
    (Frame.cc:129-132) -> ComputeStereoMatches (Frame.cc:957) -> ComputeBoW with levelsup 4 (Frame.cc:887) ->
    SearchByBoW(KF, F) (ORBmatcher.cc:226) and SearchByBoW(KF, KF) / SearchForTriangulation over the ~100 shared
    nodes, each bit-identical to the same chain on the oracle."""
    from test_gpu_stereo import rectified_pair
    ref, voc = reference_scale_vocabulary
    W, H, NF = 752, 480, 1200
    exl, exr = orb.ORBextractor(NF, 1.2, 8, 20, 7), orb.ORBextractor(NF, 1.2, 8, 20, 7)
    rl, rr = ol.OracleExtractor(NF, 1.2, 8, 20, 7), ol.OracleExtractor(NF, 1.2, 8, 20, 7)
    b = (0.0, 0.0, float(W), float(H))
    res = []
    for t in (0, 1):
        L_, R_ = rectified_pair(W, H, 77 + t, 17)
        (_, kl, dl), (_, kr, dr) = exl(L_), exr(R_)
        (_, okl, odl), (_, okr, odr) = rl(L_), rr(R_)
        assert kl.tobytes() == okl.tobytes() and np.array_equal(dl, odl) and np.array_equal(dr, odr)
        fl = orb.Frame(exl.capacity(H, W)).from_extractor(exl, 0, kl, b)
        fr = orb.Frame(exr.capacity(H, W)).from_extractor(exr, 0, kr, b)
        ur, dep = orb.ComputeStereoMatches_resident(exl, 0, exr, 0, fl, fr, 0.11, 47.9)
        our, odep = ol.stereo_matches(rl, rr, kl, dl, kr, dr, 0.11, 47.9)
        assert (our >= 0).sum() > 100 and ur.tobytes() == our.tobytes() and dep.tobytes() == odep.tobytes()
        bow, obow = fl.ComputeBoW(voc, 4), ref.transform(dl, 4)
        assert np.array_equal(bow["bow_ids"], obow["bow_ids"])
        assert np.array_equal(bow["bow_vals"].view(np.uint64), obow["bow_vals"].view(np.uint64))
        assert all(np.array_equal(x, y) for x, y in zip(bow["fv"], obow["fv"])) and len(obow["fv"][0]) > 50
        res.append((fl, kl, dl, bow["fv"], our))
    (f0, k0, d0, fv0, ur0), (f1, k1, d1, fv1, _) = res
    # the second pair is another scene: descriptors of the first one with a few flipped bits stand in for the tracked
    # frame so that SearchByBoW has real matches to find across the shared nodes
    rng = np.random.default_rng(5)
    d1m = d0.copy()
    flip = rng.integers(0, 256, (len(d1m), 6))
    for j in range(flip.shape[1]):
        d1m[np.arange(len(d1m)), flip[:, j] >> 3] ^= (1 << (flip[:, j] & 7)).astype(np.uint8)
    f1m = orb.Frame(exl.capacity(H, W)).upload(k0, d1m, b)
    fv1m, ofv1m = f1m.ComputeBoW(voc, 4)["fv"], ref.transform(d1m, 4)["fv"]
    assert all(np.array_equal(x, y) for x, y in zip(fv1m, ofv1m))
    valid = (ur0 >= 0).astype(np.uint8)  # "has a map point": the stereo-matched features
    got = f0.SearchByBoW_KF_F(valid, fv0, f1m, fv1m, 0.7, True)
    want = ol.search_by_bow_kf_f(d0, k0["angle"], valid, fv0, d1m, k0["angle"], ofv1m, 0.7, True)
    assert want[0] > 100 and got[0] == want[0] and np.array_equal(got[1], want[1])
    # round 6: both FeatureVectors are resident since the ComputeBoW calls above (Frame::mFeatVec) -- joined on the device
    got_r = f0.SearchByBoW_KF_F(valid, None, f1m, None, 0.7, True)
    assert got_r[0] == want[0] and np.array_equal(got_r[1], want[1])
    v2 = np.ones(len(k0), np.uint8)
    got = f0.SearchByBoW_KF_KF(valid, fv0, f1m, v2, fv1m, 0.8, True)
    want = ol.search_by_bow_kf_kf(d0, k0["angle"], valid, fv0, d1m, k0["angle"], v2, ofv1m, 0.8, True)
    assert want[0] > 100 and got[0] == want[0] and np.array_equal(got[1], want[1])
    got_r = f0.SearchByBoW_KF_KF(valid, None, f1m, v2, None, 0.8, True)
    assert got_r[0] == want[0] and np.array_equal(got_r[1], want[1])
    e1 = (ur0 < 0).astype(np.uint8)      # no map point yet
    got = f0.SearchForTriangulation(e1, fv0, f1m, v2, fv1m, True)
    want = ol.search_for_triangulation(d0, k0["angle"], e1, fv0, d1m, k0["angle"], v2, ofv1m, None, None, True)
    assert want[0] > 50 and got[0] == want[0] and np.array_equal(got[1], want[1])


def test_c3_chain_extract_bow_search(frames):
    """Config C3: extraction (GPU) -> ComputeBoW (GPU) -> SearchByBoW(KF, F) (GPU) == the same chain on the oracle."""
    (k0, d0), (k1, d1) = frames
    ex = orb.ORBextractor(1200, 1.2, 8, 20, 7, max_batch=2)
    outs = ex.extract_batch(np.stack([synth.sequence_frame(752, 480, 13, 0), synth.sequence_frame(752, 480, 13, 1)]))
    assert outs[0][1].tobytes() == k0.tobytes() and np.array_equal(outs[1][2], d1)
    blob = synth.synthetic_vocabulary(10, 4, seed=5)
    ref, voc = ol.OracleVocabulary(blob), orb.ORBVocabulary(blob)
    fv_kf, fv_f = voc.transform(outs[0][2], 2)["fv"], voc.transform(outs[1][2], 2)["fv"]
    rfv_kf, rfv_f = ref.transform(d0, 2)["fv"], ref.transform(d1, 2)["fv"]
    for a, b in zip(fv_kf + fv_f, rfv_kf + rfv_f):
        assert np.array_equal(a, b)
    valid = np.ones(len(d0), np.uint8)
    m = orb.ORBmatcher(0.7, True)
    n_got, got = m.SearchByBoW_KF_F(outs[0][2], outs[0][1]["angle"], valid, fv_kf, outs[1][2], outs[1][1]["angle"], fv_f)
    n_want, want = ol.search_by_bow_kf_f(d0, k0["angle"], valid, rfv_kf, d1, k1["angle"], rfv_f, 0.7, True)
    assert n_got == n_want and np.array_equal(got, want)
    assert n_want > 100


def test_resident_feature_vector_needs_its_compute_bow(reference_scale_vocabulary):
    """SearchByBoW with NULL FeatureVector arrays joins what ComputeBoW left in the frames; a frame whose features were
    written after its last ComputeBoW (or that never had one) is refused, not searched with a stale FeatureVector."""
    ref, voc = reference_scale_vocabulary
    e = ol.OracleExtractor(600, 1.2, 8, 20, 7)
    _, k0, d0 = e(synth.sequence_frame(640, 480, 21, 0))
    _, k1, d1 = e(synth.sequence_frame(640, 480, 21, 1))
    b = (0.0, 0.0, 640.0, 480.0)
    f0, f1 = orb.Frame(700).upload(k0, d0, b), orb.Frame(700).upload(k1, d1, b)
    valid = np.ones(len(k0), np.uint8)
    with pytest.raises(orb.VsgError):
        f0.SearchByBoW_KF_F(valid, None, f1, None, 0.7, True)
    fv0, fv1 = f0.ComputeBoW(voc, 4)["fv"], f1.ComputeBoW(voc, 4)["fv"]
    want = ol.search_by_bow_kf_f(d0, k0["angle"], valid, ref.transform(d0, 4)["fv"], d1, k1["angle"], ref.transform(d1, 4)["fv"],
                                 0.7, True)
    got = f0.SearchByBoW_KF_F(valid, None, f1, None, 0.7, True)
    assert want[0] > 50 and got[0] == want[0] and np.array_equal(got[1], want[1])
    f1.upload(k0, d0, b)          # new features: the resident FeatureVector is stale
    with pytest.raises(orb.VsgError):
        f0.SearchByBoW_KF_F(valid, None, f1, None, 0.7, True)


@pytest.mark.parametrize("scoring,weighting", [(0, 0), (1, 1), (5, 0), (2, 2), (0, 3)])
def test_bow_assembly_on_the_device_and_on_the_host_agree_with_the_oracle(scoring, weighting):
    """Frames of up to 2048 features are ranked by k_bow_rank and assembled by k_bow_assemble (sums in the reference's order);
    larger ones by the same steps on the host.  Both against the oracle, bit for bit, incl. stopped words (a third of the
    leaves weigh 0 here) and features that share a word (descriptors repeated)."""
    blob = synth.synthetic_vocabulary(6, 3, seed=91, scoring=scoring, weighting=weighting, stop_fraction=0.3)
    ref, voc = ol.OracleVocabulary(blob), orb.ORBVocabulary(blob)
    for n in (1, 2, 63, 1024, 2047, 2048, 2049, 3000):
        d = synth.random_descriptors(n, 700 + n)
        d[1::3] = d[0]                     # many features in one word: the running sum of addWeight
        want, got = ref.transform(d, 1), voc.transform(d, 1)
        for key in ("word", "node", "bow_ids"):
            assert np.array_equal(got[key], want[key]), (n, key)
        assert np.array_equal(got["bow_vals"].view(np.uint64), want["bow_vals"].view(np.uint64)), n
        for a, b_ in zip(got["fv"], want["fv"]):
            assert np.array_equal(a, b_), n


def test_stereo_bow_search_in_one_wait_is_the_three_blocking_calls(reference_scale_vocabulary):
    """vsg_frame_stereo_bow_search (round 6): ComputeStereoMatches + ComputeBoW + SearchByBoW(KF, F) of a stereo Frame as one
    enqueue and one wait.  Every output against the oracle's chain and against the three blocking calls, over three pairs
    (the first has no KeyFrame to search)."""
    from test_gpu_stereo import rectified_pair
    ref, voc = reference_scale_vocabulary
    W, H, NF = 752, 480, 1200
    exl, exr = orb.ORBextractor(NF, 1.2, 8, 20, 7), orb.ORBextractor(NF, 1.2, 8, 20, 7)
    rl, rr = ol.OracleExtractor(NF, 1.2, 8, 20, 7), ol.OracleExtractor(NF, 1.2, 8, 20, 7)
    b = (0.0, 0.0, float(W), float(H))
    cap = exl.capacity(H, W)
    FL, FR = [orb.Frame(cap), orb.Frame(cap)], orb.Frame(cap)
    prev = None
    for t in range(3):
        L_, R_ = rectified_pair(W, H, 77, 17 + t)
        (_, kl, dl), (_, kr, dr) = exl(L_), exr(R_)
        (_, okl, odl), (_, okr, odr) = rl(L_), rr(R_)
        assert kl.tobytes() == okl.tobytes() and np.array_equal(dl, odl) and np.array_equal(dr, odr)
        cur = FL[t & 1].from_extractor(exl, 0, kl, b)
        FR.from_extractor(exr, 0, kr, b)
        our, odep = ol.stereo_matches(rl, rr, kl, dl, kr, dr, 0.11, 47.9)
        obow = ref.transform(dl, 4)
        kf, kf_valid = (prev["frame"], prev["valid"]) if prev else (None, None)
        got = orb.stereo_bow_search(exl, 0, exr, 0, cur, FR, 0.11, 47.9, voc, 4, kf, kf_valid, 0.7, True)
        assert got["u_right"].tobytes() == our.tobytes() and got["depth"].tobytes() == odep.tobytes()
        assert got["n_stereo"] == int((our >= 0).sum()) and got["n_stereo"] > 100
        assert np.array_equal(got["bow_ids"], obow["bow_ids"])
        assert np.array_equal(got["bow_vals"].view(np.uint64), obow["bow_vals"].view(np.uint64))
        assert all(np.array_equal(x, y) for x, y in zip(got["fv"], obow["fv"]))
        if prev:
            want = ol.search_by_bow_kf_f(prev["d"], prev["k"]["angle"], prev["valid"], prev["fv"], dl, kl["angle"], obow["fv"],
                                         0.7, True)
            assert got["n_match"] == want[0] and np.array_equal(got["match_f"], want[1])
            # ... and the three blocking calls on the same frames
            ur3, dep3 = orb.ComputeStereoMatches_resident(exl, 0, exr, 0, cur, FR, 0.11, 47.9)
            bow3 = cur.ComputeBoW(voc, 4)
            m3 = prev["frame"].SearchByBoW_KF_F(prev["valid"], prev["fv"], cur, bow3["fv"], 0.7, True)
            assert ur3.tobytes() == got["u_right"].tobytes() and dep3.tobytes() == got["depth"].tobytes()
            assert np.array_equal(bow3["bow_vals"].view(np.uint64), got["bow_vals"].view(np.uint64))
            assert m3[0] == got["n_match"] and np.array_equal(m3[1], got["match_f"])
        prev = dict(frame=cur, valid=(our >= 0).astype(np.uint8), d=dl, k=kl, fv=obow["fv"])
