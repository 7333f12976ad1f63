"""SearchByBoW on the FeatureVectors that ComputeBoW leaves resident in the frames (vsg_frame_search_by_bow_kf_f / _kf_kf with
every FeatureVector array NULL: the join of ORBmatcher.cc:247-405 / 786-870 runs inside k_search_by_bow) at the shapes where
that path takes other branches: nodes on either side of the LDS distance matrix's 128 features, FeatureVectors of more than
256 nodes, fisheye stereo Frames, stopped words, empty frames and vocabularies, frames of more than 2048 features (assembled
on the host), every writer that makes a FeatureVector stale, and vsg_frame_stereo_bow_search around all of these.  Every
result is compared with the CPU oracle (and, where it applies, with the host-array form) exactly."""
import struct

import numpy as np
import pytest

import oracle_lib as ol
from bow_scenes import B, keypoints, near_dups
from visual_sgraphs_amd import orb, synth

pytestmark = pytest.mark.gpu

RATIOS = [(0.6, True), (0.75, False), (0.9, True)]


@pytest.fixture(scope="module")
def small_vocab():
    """k = 6, L = 3 with a fifth of the words stopped: levelsup 2 puts the FeatureVector at level 1 (six nodes)."""
    blob = synth.synthetic_vocabulary(6, 3, seed=31, stop_fraction=0.2)
    return ol.OracleVocabulary(blob), orb.ORBVocabulary(blob)


@pytest.fixture(scope="module")
def reference_vocab():
    """The reference's shape, k = 10, L = 6 (generated, 50 MB, never committed), with 5 % of the words stopped."""
    blob = synth.synthetic_vocabulary(10, 6, seed=17, stop_fraction=0.05)
    return ol.OracleVocabulary(blob), orb.ORBVocabulary(blob)


def rotated(angle, rng):
    """The angles a second view of the same features has: one common rotation plus a little noise."""
    return ((angle + 23.0 + rng.normal(0, 2.0, len(angle))) % 360.0).astype(np.float32)


def scene(nk, nf, seed, nleft=-1):
    """KeyFrame of nk random features; Frame of nf features, most of them near duplicates of KeyFrame features (so that
    matches, ratio-test failures and claims all happen), the rest fresh.  nleft >= 0: the Frame's first nleft features are
    the left camera's, the others the right camera's, each camera seeing the KeyFrame's features again."""
    rng = np.random.default_rng(seed)
    kd = synth.random_descriptors(nk, 1000 + seed)
    # a third of the KeyFrame's features lie close to another of its features: second-best distances near the best ones
    close = rng.random(nk) < 0.35
    kd[close] = near_dups(kd[rng.integers(0, max(nk, 1), nk)[close]], rng, 5)
    ka = rng.uniform(0, 360, nk).astype(np.float32)
    if nk == 0:
        fd, fa = synth.random_descriptors(nf, 2000 + seed), rng.uniform(0, 360, nf).astype(np.float32)
    else:
        parts = [nf] if nleft < 0 else [nleft, nf - nleft]
        src = np.concatenate([rng.permutation(max(p, nk))[:p] % nk for p in parts]).astype(np.int64)
        fd, fa = near_dups(kd[src], rng, 10), rotated(ka[src], rng)
        fresh = rng.random(nf) < 0.15
        fd[fresh] = synth.random_descriptors(int(fresh.sum()), 3000 + seed)
        turned = rng.random(nf) < 0.2  # outliers of the rotation histogram
        fa[turned] = rng.uniform(0, 360, int(turned.sum())).astype(np.float32)
    return (keypoints(ka, rng), kd), (keypoints(fa, rng), fd)


def upload(kps, desc, nleft=-1):
    return orb.Frame(max(len(kps), 1)).upload(kps, desc, B, nleft=nleft)


def fv_equal(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def check_kf_f(ref, fk, K, kfv, ff, F, ffv, valid, nnratio, ori, nleft=-1, host=True):
    """Resident KF -> F search == the oracle (== the host-array form).  Returns the oracle's result."""
    (kk, kd), (fkps, fd) = K, F
    want = ol.search_by_bow_kf_f(kd, kk["angle"], valid, kfv, fd, fkps["angle"], ffv, nnratio, ori, nleft)
    got = fk.SearchByBoW_KF_F(valid, None, ff, None, nnratio, ori)
    assert got[0] == want[0] and np.array_equal(got[1], want[1]), (nnratio, ori)
    if host:
        h = fk.SearchByBoW_KF_F(valid, kfv, ff, ffv, nnratio, ori)
        assert h[0] == want[0] and np.array_equal(h[1], want[1]), (nnratio, ori)
    return want


def check_kf_kf(ref, fk, K, kfv, ff, F, ffv, v1, v2, nnratio, ori, host=True):
    (kk, kd), (fkps, fd) = K, F
    want = ol.search_by_bow_kf_kf(kd, kk["angle"], v1, kfv, fd, fkps["angle"], v2, ffv, nnratio, ori)
    got = fk.SearchByBoW_KF_KF(v1, None, ff, v2, None, nnratio, ori)
    assert got[0] == want[0] and np.array_equal(got[1], want[1]), (nnratio, ori)
    if host:
        h = fk.SearchByBoW_KF_KF(v1, kfv, ff, v2, ffv, nnratio, ori)
        assert h[0] == want[0] and np.array_equal(h[1], want[1]), (nnratio, ori)
    return want


def resident_pair(ref, voc, levelsup, K, F, nleft=-1):
    """Both frames uploaded and their ComputeBoW run; the FeatureVectors checked against the oracle's."""
    fk, ff = upload(*K), upload(*F, nleft=nleft)
    bk, bf = fk.ComputeBoW(voc, levelsup), ff.ComputeBoW(voc, levelsup)
    ok, of = ref.transform(K[1], levelsup), ref.transform(F[1], levelsup)
    assert fv_equal(bk["fv"], ok["fv"]) and fv_equal(bf["fv"], of["fv"])
    assert np.array_equal(bk["bow_ids"], ok["bow_ids"]) and np.array_equal(bf["bow_ids"], of["bow_ids"])
    return fk, ff, ok["fv"], of["fv"]


def node_sizes(fv):
    return np.diff(fv[1])


# ---- node shapes -------------------------------------------------------------------------------------------------------

def shaped_pair(ref, levelsup, na, nb, seed):
    """A KeyFrame and a Frame that share one FeatureVector node X holding exactly na KeyFrame and nb Frame features (built
    from distinct, exactly repeated and near-duplicate descriptors, so that distances tie), next to other shared nodes, features
    of stopped words (in no node) and unrelated features."""
    rng = np.random.default_rng(seed)
    pool = synth.random_descriptors(8000, 500 + seed)
    t = ref.transform(pool, levelsup)
    live = t["weight"] > 0
    ids, cnt = np.unique(t["node"][live], return_counts=True)
    X = ids[np.argmax(cnt)]
    inX, others, stopped = pool[live & (t["node"] == X)], pool[live & (t["node"] != X)][:120], pool[~live][:25]
    nd = max(1, (2 * na) // 3)
    assert len(inX) >= nd
    kX = np.concatenate([inX[:nd], inX[rng.integers(0, nd, na - nd)]])  # a third repeated exactly
    # the Frame's node X: near duplicates of the KeyFrame's that stay in X, topped up with exact repeats of those
    def in_x(d):
        tt = ref.transform(d, levelsup)
        return (tt["weight"] > 0) & (tt["node"] == X)
    cand = near_dups(kX[np.resize(rng.permutation(na), na + nb)], rng, 6)
    cand = cand[in_x(cand)]
    assert len(cand) >= nb // 2
    fX = np.concatenate([cand, cand[rng.integers(0, len(cand), max(0, nb - len(cand)))]])[:nb]
    fO = np.concatenate([near_dups(others[rng.permutation(len(others))[:90]], rng, 6), near_dups(stopped, rng, 2),
                         synth.random_descriptors(40, 900 + seed)])
    kd = np.concatenate([kX, others, stopped])
    fd = np.concatenate([fX, fO[~in_x(fO)]])  # node X holds exactly nb Frame features
    pk, pf = rng.permutation(len(kd)), rng.permutation(len(fd))  # node X's features spread over the whole frame
    kd, fd = kd[pk], fd[pf]
    ka = rng.uniform(0, 360, len(kd)).astype(np.float32)
    fa = rng.uniform(0, 360, len(fd)).astype(np.float32)
    # a Frame feature copied from a KeyFrame feature gets its angle, rotated: the orientation filter keeps most matches
    for i in range(len(fd)):
        j = np.nonzero(np.unpackbits(kd ^ fd[i], axis=1).sum(axis=1) <= 10)[0]
        if len(j):
            fa[i] = rotated(ka[j[:1]], rng)[0]
    return (keypoints(ka, rng), kd), (keypoints(fa, rng), fd), X


@pytest.mark.parametrize("na,nb", [(128, 128), (128, 129), (129, 128), (129, 129), (100, 260), (300, 60)])
def test_node_on_either_side_of_the_lds_matrix(small_vocab, na, nb):
    """A node of at most 128 features a side is matched on the LDS distance matrix, a larger one by the scan with claims in
    device scratch: both against the oracle, at the boundary on the KeyFrame side, the Frame side and both."""
    ref, voc = small_vocab
    K, F, X = shaped_pair(ref, 2, na, nb, seed=na * 1000 + nb)
    fk, ff, kfv, ffv = resident_pair(ref, voc, 2, K, F)
    for fv, n in ((kfv, na), (ffv, nb)):
        pos = int(np.searchsorted(fv[0], X))
        assert fv[0][pos] == X and node_sizes(fv)[pos] == n
    rng = np.random.default_rng(na + nb)
    valid = (rng.random(len(K[1])) > 0.2).astype(np.uint8)
    v2 = (rng.random(len(F[1])) > 0.2).astype(np.uint8)
    total = 0
    for nnratio, ori in RATIOS:
        w = check_kf_f(ref, fk, K, kfv, ff, F, ffv, valid, nnratio, ori)
        total += w[0]
        check_kf_kf(ref, fk, K, kfv, ff, F, ffv, valid, v2, nnratio, ori)
    assert total > 60


def test_one_node_holding_every_feature(small_vocab):
    """levelsup >= L: every feature of a non-stopped word sits in the root node (DBoW2 transform, nid_level <= 0)."""
    ref, voc = small_vocab
    K, F = scene(700, 650, seed=3)
    fk, ff, kfv, ffv = resident_pair(ref, voc, 3, K, F)
    assert len(kfv[0]) == 1 and len(ffv[0]) == 1 and node_sizes(kfv)[0] > 500
    valid = np.ones(700, np.uint8)
    valid[::5] = 0
    v2 = np.ones(650, np.uint8)
    v2[::7] = 0
    for nnratio, ori in RATIOS:
        assert check_kf_f(ref, fk, K, kfv, ff, F, ffv, valid, nnratio, ori)[0] > 100
        check_kf_kf(ref, fk, K, kfv, ff, F, ffv, valid, v2, nnratio, ori)


@pytest.mark.parametrize("levelsup,n,min_nodes", [(4, 1200, 60), (3, 1500, 257)])
def test_reference_vocabulary_node_counts(reference_vocab, levelsup, n, min_nodes):
    """k = 10, L = 6: levelsup 4 is the reference's shape (~100 nodes of ~10 features); levelsup 3 gives FeatureVectors of
    more than 256 nodes, which the join reads in several passes of 256."""
    ref, voc = reference_vocab
    K, F = scene(n, n - 100, seed=levelsup * 10)
    fk, ff, kfv, ffv = resident_pair(ref, voc, levelsup, K, F)
    assert len(kfv[0]) >= min_nodes and len(ffv[0]) >= min_nodes
    rng = np.random.default_rng(levelsup)
    valid = (rng.random(n) > 0.3).astype(np.uint8)
    v2 = (rng.random(n - 100) > 0.1).astype(np.uint8)
    for nnratio, ori in RATIOS:
        assert check_kf_f(ref, fk, K, kfv, ff, F, ffv, valid, nnratio, ori)[0] > 100
        check_kf_kf(ref, fk, K, kfv, ff, F, ffv, valid, v2, nnratio, ori)


# ---- frame kinds and sizes -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nk,nleft,nright", [(700, 600, 500), (1800, 1300, 1200)])
def test_fisheye_stereo_frame(reference_vocab, nk, nleft, nright):
    """F.Nleft != -1 (ORBmatcher.cc:277-326, 362-389) through the resident join, the second size above 2048 features in all:
    a KeyFrame feature claims one feature of each camera, the right one without a ratio test."""
    ref, voc = reference_vocab
    K, F = scene(nk, nleft + nright, seed=nleft, nleft=nleft)
    fk, ff, kfv, ffv = resident_pair(ref, voc, 4, K, F, nleft=nleft)
    valid = (np.random.default_rng(nk).random(nk) > 0.2).astype(np.uint8)
    for nnratio, ori in RATIOS:
        w = check_kf_f(ref, fk, K, kfv, ff, F, ffv, valid, nnratio, ori, nleft=nleft)
        assert (w[1][:nleft] >= 0).sum() > 50 and (w[1][nleft:] >= 0).sum() > 50  # both cameras really matched


@pytest.mark.parametrize("nk,nf", [(0, 500), (500, 0), (0, 0), (1, 1), (1, 400), (400, 1), (2, 2), (2047, 2047),
                                   (2048, 2048), (2048, 2049), (2049, 2048), (2049, 2049), (3000, 3000), (3000, 600),
                                   (600, 3000)])
def test_frame_sizes(reference_vocab, nk, nf):
    """Frames of 0, 1, 2 and 2047 / 2048 / 2049 / 3000 features: empty frames give 0 matches (the reference's empty join),
    frames above 2048 features have their FeatureVector assembled on the host and copied into the frame."""
    ref, voc = reference_vocab
    K, F = scene(nk, nf, seed=nk * 7 + nf)
    fk, ff, kfv, ffv = resident_pair(ref, voc, 4, K, F)
    rng = np.random.default_rng(nk + nf)
    valid = (rng.random(nk) > 0.2).astype(np.uint8)
    v2 = (rng.random(nf) > 0.1).astype(np.uint8)
    for nnratio, ori in RATIOS:
        w = check_kf_f(ref, fk, K, kfv, ff, F, ffv, valid, nnratio, ori)
        w2 = check_kf_kf(ref, fk, K, kfv, ff, F, ffv, valid, v2, nnratio, ori)
        if min(nk, nf) >= 2000:
            assert w[0] > 300 and w2[0] > 200
        if min(nk, nf) == 0:
            assert w[0] == w2[0] == 0 and np.all(w[1] == -1) and np.all(w2[1] == -1)


def test_empty_vocabulary(small_vocab):
    """A vocabulary image of the 16-byte header alone is DBoW2's empty(): loaded by both, transform gives empty vectors and
    SearchByBoW finds nothing -- 0 matches, every output -1."""
    blob = struct.pack("<iiii", 10, 6, 0, 0)
    ref, voc = ol.OracleVocabulary(blob), orb.ORBVocabulary(blob)
    assert (voc.k, voc.L, voc.nnodes, voc.nwords) == (ref.k, ref.L, ref.nnodes, ref.nwords) == (10, 6, 1, 0)
    K, F = scene(500, 300, seed=9)
    fk, ff, kfv, ffv = resident_pair(ref, voc, 4, K, F)
    assert len(kfv[0]) == len(ffv[0]) == 0
    valid, v2 = np.ones(500, np.uint8), np.ones(300, np.uint8)
    for nnratio, ori in RATIOS:
        w = check_kf_f(ref, fk, K, kfv, ff, F, ffv, valid, nnratio, ori)
        w2 = check_kf_kf(ref, fk, K, kfv, ff, F, ffv, valid, v2, nnratio, ori)
        assert w[0] == w2[0] == 0 and np.all(w[1] == -1) and np.all(w2[1] == -1)
    # the frames stay usable: a ComputeBoW with a real vocabulary makes them searchable again
    sref, svoc = small_vocab
    bk, bf = fk.ComputeBoW(svoc, 2), ff.ComputeBoW(svoc, 2)
    assert check_kf_f(sref, fk, K, bk["fv"], ff, F, bf["fv"], valid, 0.75, True)[0] > 20


# ---- stale FeatureVectors --------------------------------------------------------------------------------------------

WRITERS = ["upload", "from_extractor", "from_extractor_undistort", "extract_into", "extract_into_rgbd"]


@pytest.mark.parametrize("writer", WRITERS)
def test_every_writer_makes_the_feature_vector_stale(reference_vocab, writer):
    """Writing a frame's features by any route after its ComputeBoW makes the resident search refuse it until ComputeBoW
    runs again; then the result is the oracle's on the new features."""
    ref, voc = reference_vocab
    W, H = 640, 480
    cam = ol.scaled_camera("tum1", W, H)
    K4, dist = np.asarray(cam["K4"], np.float32), np.asarray(cam["dist"], np.float32)
    ex = orb.ORBextractor(1000, 1.2, 8, 20, 7)
    oex = ol.OracleExtractor(1000, 1.2, 8, 20, 7)
    imgs = [synth.sequence_frame(W, H, 41, t) for t in range(3)]
    _, k0, d0 = oex(imgs[0])
    kf = upload(k0, d0)
    kfv = kf.ComputeBoW(voc, 4)["fv"]
    valid = np.ones(len(k0), np.uint8)
    valid[::6] = 0
    f = orb.Frame(ex.capacity(H, W))

    def write(img):
        """The frame's features through `writer`; returns (descriptors, angles) of what it now holds."""
        if writer == "upload":
            _, k, d = oex(img)
            f.upload(k, d, B)
        elif writer in ("from_extractor", "from_extractor_undistort"):
            _, k, d = ex(img)
            if writer == "from_extractor":
                f.from_extractor(ex, 0, k, B)
            else:
                f.from_extractor_undistort(ex, 0, k, K4, dist, B)
        elif writer == "extract_into":
            _, k, d = f.extract_into(ex, img, B, K4, dist)
        else:
            depth = np.full((H, W), 1500, np.uint16)
            _, k, d, _, _ = f.extract_into_rgbd(ex, img, depth, B, K4, dist, 0.001, 40.0)
        return d, f.kps["angle"].copy()

    for t in (1, 2):
        d, a = write(imgs[t])
        with pytest.raises(orb.VsgError):
            kf.SearchByBoW_KF_F(valid, None, f, None, 0.75, True)
        with pytest.raises(orb.VsgError):
            kf.SearchByBoW_KF_KF(valid, None, f, np.ones(len(d), np.uint8), None, 0.75, True)
        ffv = f.ComputeBoW(voc, 4)["fv"]
        assert fv_equal(ffv, ref.transform(d, 4)["fv"])
        want = ol.search_by_bow_kf_f(d0, k0["angle"], valid, kfv, d, a, ffv, 0.75, True)
        got = kf.SearchByBoW_KF_F(valid, None, f, None, 0.75, True)
        assert want[0] > 50 and got[0] == want[0] and np.array_equal(got[1], want[1]), t


# ---- vsg_frame_stereo_bow_search ---------------------------------------------------------------------------------------

def test_stereo_bow_search_above_2048_features(reference_vocab):
    """A stereo Frame of more than 2048 features (2500 requested per eye): ComputeBoW assembles on the host after the wait
    and the search against the KeyFrame follows; every output equals the oracle's chain and the three blocking calls."""
    from test_gpu_stereo import rectified_pair
    ref, voc = reference_vocab
    W, H, NF = 752, 480, 2500
    exl, exr = orb.ORBextractor(NF, 1.2, 8, 20, 7), orb.ORBextractor(NF, 1.2, 8, 20, 7)
    rl, rr = ol.OracleExtractor(NF, 1.2, 8, 20, 7), ol.OracleExtractor(NF, 1.2, 8, 20, 7)
    cap = exl.capacity(H, W)
    FL, FR = [orb.Frame(cap), orb.Frame(cap)], orb.Frame(cap)
    prev = None
    for t in range(3):
        L_, R_ = rectified_pair(W, H, 77, 17 + t)
        (_, kl, dl), (_, kr, dr) = exl(L_), exr(R_)
        (_, okl, odl), (_, okr, odr) = rl(L_), rr(R_)
        assert kl.tobytes() == okl.tobytes() and np.array_equal(dl, odl) and np.array_equal(dr, odr) and len(kl) > 2048
        cur = FL[t & 1].from_extractor(exl, 0, kl, (0.0, 0.0, float(W), float(H)))
        FR.from_extractor(exr, 0, kr, (0.0, 0.0, float(W), float(H)))
        our, odep = ol.stereo_matches(rl, rr, kl, dl, kr, dr, 0.11, 47.9)
        obow = ref.transform(dl, 4)
        kf, kf_valid = (prev["frame"], prev["valid"]) if prev else (None, None)
        got = orb.stereo_bow_search(exl, 0, exr, 0, cur, FR, 0.11, 47.9, voc, 4, kf, kf_valid, 0.7, True)
        assert got["u_right"].tobytes() == our.tobytes() and got["depth"].tobytes() == odep.tobytes()
        assert np.array_equal(got["bow_ids"], obow["bow_ids"])
        assert np.array_equal(got["bow_vals"].view(np.uint64), obow["bow_vals"].view(np.uint64))
        assert fv_equal(got["fv"], obow["fv"])
        if prev:
            want = ol.search_by_bow_kf_f(prev["d"], prev["k"]["angle"], prev["valid"], prev["fv"], dl, kl["angle"], obow["fv"],
                                         0.7, True)
            assert want[0] > 100 and got["n_match"] == want[0] and np.array_equal(got["match_f"], want[1])
            # the resident FeatureVector left in `cur` by the chain is searchable by the blocking form too
            m_res = prev["frame"].SearchByBoW_KF_F(prev["valid"], None, cur, None, 0.7, True)
            assert m_res[0] == want[0] and np.array_equal(m_res[1], want[1])
            # ... and the three blocking calls on the same frames
            ur3, dep3 = orb.ComputeStereoMatches_resident(exl, 0, exr, 0, cur, FR, 0.11, 47.9)
            bow3 = cur.ComputeBoW(voc, 4)
            m3 = prev["frame"].SearchByBoW_KF_F(prev["valid"], prev["fv"], cur, bow3["fv"], 0.7, True)
            assert ur3.tobytes() == got["u_right"].tobytes() and dep3.tobytes() == got["depth"].tobytes()
            assert np.array_equal(bow3["bow_vals"].view(np.uint64), got["bow_vals"].view(np.uint64))
            assert m3[0] == got["n_match"] and np.array_equal(m3[1], got["match_f"])
        prev = dict(frame=cur, valid=(our >= 0).astype(np.uint8), d=dl, k=kl, fv=obow["fv"])


def test_stereo_bow_search_refusal_leaves_nothing_running(reference_vocab):
    """A KeyFrame that never had its ComputeBoW is refused before anything is enqueued; the next calls on the same thread
    (ComputeBoW + a resident search of other frames, then the chain with a proper KeyFrame) equal the oracle."""
    from test_gpu_stereo import rectified_pair
    ref, voc = reference_vocab
    W, H, NF = 752, 480, 1200
    exl, exr = orb.ORBextractor(NF, 1.2, 8, 20, 7), orb.ORBextractor(NF, 1.2, 8, 20, 7)
    rl = ol.OracleExtractor(NF, 1.2, 8, 20, 7)
    cap = exl.capacity(H, W)
    fl, fr = orb.Frame(cap), orb.Frame(cap)
    b = (0.0, 0.0, float(W), float(H))
    L_, R_ = rectified_pair(W, H, 78, 17)
    (_, kl, dl), (_, kr, _) = exl(L_), exr(R_)
    fl.from_extractor(exl, 0, kl, b)
    fr.from_extractor(exr, 0, kr, b)
    K, F = scene(900, 800, seed=12)
    no_bow = upload(*K)
    with pytest.raises(orb.VsgError):
        orb.stereo_bow_search(exl, 0, exr, 0, fl, fr, 0.11, 47.9, voc, 4, no_bow, np.ones(900, np.uint8), 0.7, True)
    fk, ff, kfv, ffv = resident_pair(ref, voc, 4, K, F)
    valid = np.ones(900, np.uint8)
    assert check_kf_f(ref, fk, K, kfv, ff, F, ffv, valid, 0.7, True, host=False)[0] > 100
    # the refused call wrote nothing the next chain depends on: fl against a KeyFrame whose ComputeBoW ran
    kd = near_dups(dl, np.random.default_rng(4), 6)
    kf = upload(kl, kd)
    kfv2 = kf.ComputeBoW(voc, 4)["fv"]
    assert fv_equal(ref.transform(kd, 4)["fv"], kfv2)
    v = np.ones(len(kl), np.uint8)
    got = orb.stereo_bow_search(exl, 0, exr, 0, fl, fr, 0.11, 47.9, voc, 4, kf, v, 0.7, True)
    obow = ref.transform(dl, 4)
    want = ol.search_by_bow_kf_f(kd, kl["angle"], v, kfv2, dl, kl["angle"], obow["fv"], 0.7, True)
    assert np.array_equal(rl(L_)[2], dl) and fv_equal(got["fv"], obow["fv"])
    assert want[0] > 100 and got["n_match"] == want[0] and np.array_equal(got["match_f"], want[1])
