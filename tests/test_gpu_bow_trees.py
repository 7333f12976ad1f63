"""The vocabulary transform on the device (vsg_bow.hip) on the vocabularies of tests/vocab_trees.py: nodes of more than 16
children (k_bow_descend<32>: the xor-16 step of the group minimum, 8 descriptors per block, winners in lanes 16..31), nodes
of 1..32 children and leaves above depth L (the child count of NodeRec::link, the `j < cnt` mask, node 0 for a leaf above the
FeatureVector's level, the max_children-based bound the resident joins launch for), and files numbered depth-first or
scattered (pass 2 of vsg_vocab_load).  Every output is compared bit for bit with oracle/bow_oracle.cpp on the same bytes;
tests/test_vocab_trees.py holds that oracle against a third, plain walk on the same trees without a GPU.

A leaf above the FeatureVector's level (nid_level = L - levelsup > the leaf's level): the reference leaves `nid`
uninitialised there (TemplatedVocabulary.h:1163 declares it, :1263 is the only assignment).  The oracle and the kernel both
give node 0, and the tests below hold them to it.  That is deliberate -- do not "fix" either side."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

import oracle_lib as ol
import vocab_trees as vt
from bow_scenes import B, keypoints, near_dups
from visual_sgraphs_amd import orb

pytestmark = pytest.mark.gpu

NAMES = list(vt.TREES)
UNSUPPORTED = -3  # include/vsg_orb.h: VSG_ERR_UNSUPPORTED
FIELDS = ("word", "node", "bow_ids")


@lru_cache(maxsize=None)
def vocab(name, order, weighting=0, scoring=0):
    """(image, oracle, library) of one vocabulary file, loaded once."""
    img = vt.image(name, order, weighting, scoring)
    return img, ol.OracleVocabulary(img.blob), orb.ORBVocabulary(img.blob)


def same(got, want, what):
    for key in FIELDS:
        assert np.array_equal(got[key], want[key]), (what, key)
    for key in ("weight", "bow_vals"):
        assert np.array_equal(got[key].view(np.uint64), want[key].view(np.uint64)), (what, key)  # bit-identical doubles
    for a, b, key in zip(got["fv"], want["fv"], ("fv_node", "fv_off", "fv_idx")):
        assert np.array_equal(a, b), (what, key)


def frame(desc, seed=0, capacity=None):
    rng = np.random.default_rng(seed)
    k = keypoints(rng.uniform(0, 360, len(desc)).astype(np.float32), rng)
    return orb.Frame(capacity or max(len(desc), 1)).upload(k, desc, B), k


# ---- the descent -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", vt.ORDERS)
@pytest.mark.parametrize("name", NAMES)
def test_descent_equals_the_oracle(name, order):
    """Every tree in every file order, every levelsup from 0 to L + 1, on the tree's whole query set; then the feature
    counts at the edges of a group and of a block: 32 lanes a descriptor is 8 descriptors a block (n = 1, 7, 8, 9, 65), 16
    lanes is 16 (n = 15, 16, 17)."""
    img, ref, voc = vocab(name, order)
    assert (voc.k, voc.L, voc.scoring, voc.weighting, voc.nnodes, voc.nwords) == \
        (ref.k, ref.L, ref.scoring, ref.weighting, ref.nnodes, ref.nwords) == (img.k, img.L, 0, 0, img.nnodes, img.nwords)
    q = vt.queries(name)
    for levelsup in range(img.L + 2):
        want = ref.transform(q, levelsup)
        if levelsup == 0:
            vt.check_fixture(name, img, want)  # on the oracle alone, before the library runs
        same(voc.transform(q, levelsup), want, (name, order, levelsup))
    wide = img.max_children > 16
    assert wide == (name in vt.WIDE)
    tail = q[::-1]  # the nodes' own descriptors, deepest first: in the wide trees winners in lanes >= 16 among the first few
    for n in (1, 7, 8, 9, 65) if wide else (15, 16, 17):
        for src in (q, tail):
            same(voc.transform(src[:n], 1), ref.transform(src[:n], 1), (name, order, "n", n))


def test_sixteen_children_take_the_16_lane_form_and_seventeen_the_32_lane_form():
    """bow_enqueue chooses by max_children <= 16.  What can be seen from outside: the header's k, the tree's widest node,
    and that both sides of the threshold give the oracle's answer with the LAST child winning (lane 15, lane 16)."""
    for name, k in (("full_16", 16), ("full_17", 17)):
        img, ref, voc = vocab(name, "bfs")
        assert voc.k == k == img.max_children and img.nnodes == vt.capacity(k, 2)
        last = np.stack([img.desc[c[-1]] for c in img.children if c])  # the last child of every node
        want = ref.transform(last, 0)
        pos, _ = vt.positions_from_words(img, want["word"])
        assert (pos[:, 1:] == k - 1).any(0).all()  # the last lane wins at both levels
        same(voc.transform(last, 0), want, name)


def test_complement_gives_the_largest_key():
    """Distance 256 at every level of a single-child chain: (256 << 8 | 0) is the largest key a live lane holds, and it
    must still beat the idle lanes' sentinel."""
    img, ref, voc = vocab("complement", "bfs")
    q = np.repeat(vt.COMPLEMENT_QUERY[None, :], 3, axis=0)
    assert (np.unpackbits(q[0] ^ img.desc[1:], axis=1).sum(1) == 256).all()
    for levelsup in range(img.L + 2):
        want = ref.transform(q, levelsup)
        assert (want["word"] == 0).all() and (want["node"] == max(img.L - levelsup, 0)).all()
        same(voc.transform(q, levelsup), want, levelsup)


@pytest.mark.parametrize("name,order", [("ragged", "dfs"), ("wide_32", "bfs")])
def test_descent_on_a_resident_frame(name, order):
    """Frame.upload + ComputeBoW == the host-descriptor call == the oracle, byte for byte."""
    img, ref, voc = vocab(name, order)
    q = vt.queries(name)
    f, _ = frame(q)
    for levelsup in range(img.L + 2):
        want, host, res = ref.transform(q, levelsup), voc.transform(q, levelsup), f.ComputeBoW(voc, levelsup)
        same(res, want, (name, levelsup))
        for key in FIELDS + ("weight", "bow_vals"):
            assert res[key].tobytes() == host[key].tobytes(), key
        assert all(a.tobytes() == b.tobytes() for a, b in zip(res["fv"], host["fv"]))


# ---- the resident joins on irregular FeatureVectors ------------------------------------------------------------------

def all_pairs_pass(n_levels=8):
    """Arguments of SearchForTriangulationEpipolar under which the geometry rejects no pair (bCoarse, mono frames, the
    epipole far away): what is left is the join of the two resident FeatureVectors and the descriptor search.  This form
    stands in for SearchForTriangulation because it is the one entry point that joins resident FeatureVectors (NULL arrays);
    vsg_frame_search_for_triangulation takes host arrays only.  The oracle is the plain search with every pair allowed."""
    sf = (np.float32(1.2) ** np.arange(n_levels, dtype=np.float32)).astype(np.float32)
    return (np.eye(3, dtype=np.float32), np.array([1e6, 1e6], np.float32), sf, (sf * sf).astype(np.float32), False, True)


def joins_equal_the_oracle(ref, voc, levelsup, d1, d2, seed, at_least):
    f1, k1 = frame(d1, seed)
    f2, k2 = frame(d2, seed + 1)
    fv1, fv2 = ref.transform(d1, levelsup)["fv"], ref.transform(d2, levelsup)["fv"]
    same(f1.ComputeBoW(voc, levelsup), ref.transform(d1, levelsup), "frame 1")
    same(f2.ComputeBoW(voc, levelsup), ref.transform(d2, levelsup), "frame 2")
    rng = np.random.default_rng(seed)
    v1 = (rng.random(len(d1)) > 0.15).astype(np.uint8)
    v2 = (rng.random(len(d2)) > 0.15).astype(np.uint8)
    found = []
    for nnratio, ori in ((0.75, True), (0.9, False)):
        want = ol.search_by_bow_kf_f(d1, k1["angle"], v1, fv1, d2, k2["angle"], fv2, nnratio, ori)
        got = f1.SearchByBoW_KF_F(v1, None, f2, None, nnratio, ori)
        assert got[0] == want[0] and np.array_equal(got[1], want[1]), ("kf_f", levelsup, nnratio)
        want2 = ol.search_by_bow_kf_kf(d1, k1["angle"], v1, fv1, d2, k2["angle"], v2, fv2, nnratio, ori)
        got2 = f1.SearchByBoW_KF_KF(v1, None, f2, v2, None, nnratio, ori)
        assert got2[0] == want2[0] and np.array_equal(got2[1], want2[1]), ("kf_kf", levelsup, nnratio)
        want3 = ol.search_for_triangulation(d1, k1["angle"], v1, fv1, d2, k2["angle"], v2, fv2, None, None, ori)
        got3 = f1.SearchForTriangulationEpipolar(v1, f2, v2, *all_pairs_pass(), ori)
        assert got3[0] == want3[0] and np.array_equal(got3[1], want3[1]), ("triangulation", levelsup)
        found.append((want[0], want2[0], want3[0]))
    assert min(min(f) for f in found) >= at_least, found  # an empty join cannot pass
    return fv1, fv2


@pytest.mark.parametrize("levelsup", [2, 0])
def test_resident_joins_on_a_ragged_depth_first_vocabulary(levelsup):
    """SearchByBoW(KF, F), SearchByBoW(KF, KF) and SearchForTriangulation with NULL FeatureVector arrays -- the join on the
    device -- after ComputeBoW with ragged/dfs.  levelsup 2 (nid_level 2): the node-0 bucket of the leaves above level 2
    lies beside real level-2 nodes whose ids are sparse and large in the depth-first file.  levelsup 0 (nid_level 4 = L):
    most nodes hold one feature."""
    img, ref, voc = vocab("ragged", "dfs")
    d1 = vt.queries("ragged")
    d2 = near_dups(d1, np.random.default_rng(77), 4)
    fv1, fv2 = joins_equal_the_oracle(ref, voc, levelsup, d1, d2, 40 + levelsup, at_least=21)
    sizes = np.diff(fv1[1])
    if levelsup == 2:
        assert fv1[0][0] == 0 and fv2[0][0] == 0 and sizes[0] >= 5   # the node-0 bucket
        assert set(img.level[fv1[0][1:]]) == {2} and fv1[0].max() > 400 and len(fv1[0]) >= 30
    else:
        assert fv1[0][0] == 0 and np.median(sizes[1:]) == 1 and len(fv1[0]) >= 300


def test_feature_vector_bound_is_tight():
    """5 features in 5 different level-1 nodes of a tree whose widest node has 10 children, FeatureVector at level 1: n_fv =
    n = 5 and the bound the joins launch for is min(10^1, 5) = 5 -- one node more than that would go unsearched."""
    img, ref, voc = vocab("ragged", "dfs")
    assert img.max_children == 10 and img.L == 4
    q = vt.queries("ragged")
    t = ref.transform(q, 3)
    live = np.flatnonzero(t["weight"] > 0)
    nodes, first = np.unique(t["node"][live], return_index=True)
    assert len(nodes) == 9 and set(img.level[nodes]) == {1}  # the tenth level-1 node is a stopped leaf
    assert nodes[-1] == img.children[0][9]
    d1 = q[live[first[[0, 2, 4, 6, 8]]]]  # the fifth feature sits in the LAST level-1 node
    d2 = d1[::-1].copy()  # the same five features, last first
    fv1, fv2 = joins_equal_the_oracle(ref, voc, 3, d1, d2, 3, at_least=0)
    assert len(fv1[0]) == len(fv2[0]) == 5 and np.array_equal(fv1[0], fv2[0])
    f1, k1 = frame(d1, 1)
    f2, k2 = frame(d2, 2)
    f1.ComputeBoW(voc, 3), f2.ComputeBoW(voc, 3)
    one = np.ones(5, np.uint8)
    want = ol.search_by_bow_kf_f(d1, k1["angle"], one, fv1, d2, k2["angle"], fv2, 0.9, False)
    got = f1.SearchByBoW_KF_F(one, None, f2, None, 0.9, False)
    assert want[0] == 5 and got[0] == 5 and np.array_equal(got[1], want[1]) and np.array_equal(want[1], [4, 3, 2, 1, 0])
    want = ol.search_for_triangulation(d1, k1["angle"], one, fv1, d2, k2["angle"], one, fv2, None, None, False)
    got = f1.SearchForTriangulationEpipolar(one, f2, one, *all_pairs_pass(), False)
    assert want[0] == 5 and got[0] == 5 and np.array_equal(got[1], want[1])


# ---- assembly edges ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("weighting,scoring", vt.PAIRS)
def test_assembly_sizes_at_the_rank_and_scan_edges(weighting, scoring):
    """n = 0, 16, 17 (J = ceil(n / 16) of k_bow_rank goes 0, 1, 2), 64, 65 (its 64-key block), 1023, 1025 (the first use of
    a thread's second element in k_bow_assemble), with stopped words and features that share a word."""
    img, ref, voc = vocab("ragged", "dfs", weighting, scoring)
    pool = np.resize(vt.queries("ragged"), (1025, 32))
    pool = pool[np.random.default_rng(9).permutation(1025)]
    pool[1::3] = pool[0]  # many features in one word: the running sum of addWeight
    for n in (0, 16, 17, 64, 65, 1023, 1025):
        want = ref.transform(pool[:n], 2)
        assert n == 0 or (0 < (want["weight"] > 0).sum() and (n < 64 or (want["weight"] <= 0).any()))
        same(voc.transform(pool[:n], 2), want, (weighting, scoring, n))


def test_every_feature_in_a_stopped_word():
    """m = 0: n_bow = n_fv = 0, fv_off[0] = 0, and a frame holding that empty FeatureVector is searchable: 0 matches."""
    img, ref, voc = vocab("ragged", "dfs")
    q = vt.queries("ragged")
    t = ref.transform(q, 2)
    stopped = q[~(t["weight"] > 0)]
    assert len(stopped) >= 40
    d = np.resize(stopped, (100, 32))
    want = ref.transform(d, 2)
    assert len(want["bow_ids"]) == 0 and len(want["fv"][0]) == 0 and not (want["weight"] > 0).any()
    got = voc.transform(d, 2)
    same(got, want, "stopped")
    assert len(got["bow_ids"]) == len(got["bow_vals"]) == len(got["fv"][0]) == len(got["fv"][2]) == 0
    assert got["fv"][1].tolist() == [0]
    f0, k0 = frame(d, 1)
    same(f0.ComputeBoW(voc, 2), want, "stopped, resident")
    live = q[t["weight"] > 0][:200]
    f1, k1 = frame(live, 2)
    fv1 = f1.ComputeBoW(voc, 2)["fv"]
    assert len(fv1[0]) > 10
    v0, v1 = np.ones(100, np.uint8), np.ones(200, np.uint8)
    for a, va, b, vb in ((f0, v0, f1, v1), (f1, v1, f0, v0), (f0, v0, f0, v0)):
        nm, m = a.SearchByBoW_KF_F(va, None, b, None, 0.9, False)
        assert nm == 0 and len(m) == b.N and (m == -1).all()
        nm, m = a.SearchByBoW_KF_KF(va, None, b, vb, None, 0.9, False)
        assert nm == 0 and len(m) == a.N and (m == -1).all()
        nm, m = a.SearchForTriangulationEpipolar(va, b, vb, *all_pairs_pass(), False)
        assert nm == 0 and len(m) == a.N and (m == -1).all()
    # the same frame is searchable with matches once it holds live features again
    f0.upload(k1[:100], live[:100], B)
    f0.ComputeBoW(voc, 2)
    want = ol.search_by_bow_kf_f(live[:100], k1["angle"][:100], v0, ref.transform(live[:100], 2)["fv"], live, k1["angle"], fv1,
                                 0.9, False)
    got = f0.SearchByBoW_KF_F(v0, None, f1, None, 0.9, False)
    assert want[0] > 20 and got[0] == want[0] and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("weighting,scoring", [(0, 0), (0, 5), (2, 0), (2, 5)])
def test_2048_features_in_one_word(weighting, scoring):
    """Under TF_IDF the head thread adds the word's weight 2047 times, left to right: the bits of the sum are the oracle's
    (the dot-product scoring leaves it unnormalised, so it is the sum itself that is compared).  Under IDF the first
    feature's weight stands.  One feature of another word keeps the L1 norm from hiding the sum."""
    img, ref, voc = vocab("ragged", "dfs", weighting, scoring)
    q = vt.queries("ragged")
    t = ref.transform(q, 2)
    live = np.flatnonzero(t["weight"] > 0)
    a = live[0]
    b = live[t["word"][live] != t["word"][a]][0]
    for d in (np.repeat(q[a][None, :], 2048, axis=0), np.concatenate([np.repeat(q[a][None, :], 2047, axis=0), q[b][None, :]])):
        want = ref.transform(d, 2)
        assert len(want["bow_ids"]) == len(np.unique(want["word"])) <= 2
        if scoring == 5 and len(want["bow_ids"]) == 1:
            w = float(t["weight"][a])
            chain = w
            for _ in range(2047):
                chain += w
            assert want["bow_vals"][0] == (chain if weighting == 0 else w)
        same(voc.transform(d, 2), want, (weighting, scoring, len(np.unique(want["word"]))))


def test_2048_features_in_2048_words():
    """Every sorted position is a group head: the scans of k_bow_assemble at their widest.  full_20_L3 has 8000 words; the
    oracle places a larger seeded set and the first feature of each live word is kept."""
    img, ref, voc = vocab("full_20_L3", "scattered")
    q = vt.queries("full_20_L3")
    t = ref.transform(q, 1)
    live = np.flatnonzero(t["weight"] > 0)
    words, first = np.unique(t["word"][live], return_index=True)
    assert len(words) >= 2048  # before the library runs
    pick = np.sort(live[first])[:2048]
    d = q[pick][np.random.default_rng(2048).permutation(2048)]
    for levelsup in (0, 1):  # 2048 FeatureVector nodes too, then ~400
        want = ref.transform(d, levelsup)
        assert len(want["bow_ids"]) == 2048 and len(want["fv"][0]) == (2048 if levelsup == 0 else len(np.unique(want["node"])))
        same(voc.transform(d, levelsup), want, levelsup)


@pytest.mark.parametrize("stopped_at", [1023, 1024])
def test_stopped_and_live_features_at_the_seam_of_a_thread_s_two_elements(stopped_at):
    """Thread t of k_bow_assemble loads features t and t + 1024: a stopped feature at 1023 with a live one at 1024, and the
    reverse, in a frame whose other features are a mix."""
    img, ref, voc = vocab("ragged", "dfs")
    q = vt.queries("ragged")
    t = ref.transform(q, 2)
    live, stopped = q[t["weight"] > 0], q[~(t["weight"] > 0)]
    d = np.resize(q, (1100, 32)).copy()
    d[1023], d[1024] = (stopped[0], live[0]) if stopped_at == 1023 else (live[0], stopped[0])
    for n in (1025, 1100):
        want = ref.transform(d[:n], 2)
        assert (want["weight"][1023] > 0) == (stopped_at != 1023) and (want["weight"][1024] > 0) == (stopped_at != 1024)
        same(voc.transform(d[:n], 2), want, (stopped_at, n))


# ---- refusal -----------------------------------------------------------------------------------------------------------

def test_a_node_of_33_children_is_refused_and_the_next_load_works():
    img = vt.image("wide_33", "bfs")
    assert img.max_children == 33
    with pytest.raises(orb.VsgError) as e:
        orb.ORBVocabulary(img.blob)
    assert e.value.code == UNSUPPORTED
    L = orb.load_library()  # ... and no handle comes back
    b = np.frombuffer(img.blob, np.uint8).copy()
    h = C.c_void_p(0xDEAD)
    assert L.vsg_vocab_load(0, b.ctypes.data_as(C.POINTER(C.c_uint8)), len(b), C.byref(h)) == UNSUPPORTED and not h.value
    good = vt.image("wide_32", "scattered", 1, 1)
    ref, voc = ol.OracleVocabulary(good.blob), orb.ORBVocabulary(good.blob)
    q = vt.queries("wide_32")
    same(voc.transform(q, 2), ref.transform(q, 2), "after the refusal")
    voc.close()
