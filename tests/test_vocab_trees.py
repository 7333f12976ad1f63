"""The CPU oracle of the vocabulary transform (oracle/bow_oracle.cpp) against a THIRD answer, on the vocabularies a trained
DBoW2 file can hold and synth.synthetic_vocabulary never makes (tests/vocab_trees.py): nodes of 1..32 children, leaves
above depth L, and files numbered depth-first (HKmeansStep's order) or in a scattered parent-before-child order.

The oracle's loader and the library's were written side by side; the third answer is vocab_trees.transform_py, a plain
NumPy / Python-float walk of the tree the builder RETURNS (never parsed back from the bytes).  Equal means equal: word,
node, BowVector ids and the FeatureVector as integers, weights and BowVector values as uint64 bit patterns.

A leaf above the FeatureVector's level (nid_level = L - levelsup > the leaf's level): the reference leaves `nid`
uninitialised there (TemplatedVocabulary.h:1163 declares it, :1263 is the only assignment).  The oracle, the kernel and
the walk all give node 0.  That is deliberate -- do not "fix" either side towards anything else."""
import numpy as np
import pytest

import oracle_lib as ol
import vocab_trees as vt

NAMES = list(vt.TREES)


@pytest.fixture(scope="module")
def walked():
    """descend() once per (tree, order): the walk does not depend on levelsup, weighting or scoring."""
    cache = {}

    def get(name, order):
        if (name, order) not in cache:
            cache[name, order] = vt.descend(vt.image(name, order), vt.queries(name))
        return cache[name, order]
    return get


def same(got, want, what):
    for key in ("word", "node", "bow_ids"):
        assert np.array_equal(got[key], want[key]), (what, key)
    for key in ("weight", "bow_vals"):
        assert np.array_equal(got[key].view(np.uint64), want[key].view(np.uint64)), (what, key)
    for a, b, key in zip(got["fv"], want["fv"], ("fv_node", "fv_off", "fv_idx")):
        assert np.array_equal(a, b), (what, key)


@pytest.mark.parametrize("order", vt.ORDERS)
@pytest.mark.parametrize("name", NAMES)
def test_oracle_equals_the_plain_walk(walked, name, order):
    q = vt.queries(name)
    w = walked(name, order)
    for weighting, scoring in vt.PAIRS:
        img = vt.image(name, order, weighting, scoring)
        ref = ol.OracleVocabulary(img.blob)
        assert (ref.k, ref.L, ref.scoring, ref.weighting, ref.nnodes, ref.nwords) == \
            (img.k, img.L, scoring, weighting, img.nnodes, img.nwords)
        for levelsup in range(img.L + 2):
            want = vt.transform_py(img, q, levelsup, w)
            got = ref.transform(q, levelsup)
            same(got, want, (name, order, weighting, scoring, levelsup))
            if (weighting, scoring) == (0, 0) and levelsup == 0:
                pos, leaf = vt.check_fixture(name, img, got)  # on the oracle's words, through the builder's tree
                assert np.array_equal(pos, w[1]) and np.array_equal(leaf, w[2])
    # node 0 for shallow leaves really happens where the tree has them, beside real nodes of that level
    img = vt.image(name, order)
    if name == "ragged":
        t = vt.transform_py(img, q, 2, w)  # nid_level = 2
        live = t["weight"] > 0
        assert (t["node"][live] == 0).sum() >= 5 and (t["node"][live] > 0).sum() >= 100
        assert set(img.level[np.unique(t["node"][t["node"] > 0])]) == {2}


SHAPES = {  # max children, leaves per level 1.., words
    "full_16": (16, [0, 256], 256),
    "full_17": (17, [0, 289], 289),
    "full_20": (20, [0, 400], 400),
    "wide_32": (32, [0, 528, 0], 528),
    "ties_wide": (20, [0, 400], 400),
    "complement": (1, [0, 0, 0, 1], 1),
    "full_20_L3": (20, [0, 0, 8000], 8000),
}


@pytest.mark.parametrize("name", NAMES + list(vt.REFUSED))
def test_tree_shapes(name):
    imgs = [vt.image(name, o) for o in vt.ORDERS]
    t = vt.tree(name)
    for img in imgs:
        per_level = np.bincount(img.level[img.is_leaf], minlength=img.L + 1)[1:].tolist()
        counts = np.array([len(c) for c in img.children])
        assert img.max_children == counts.max() and img.nwords == img.is_leaf.sum() == sum(per_level)
        assert len(img.blob) == 16 + 45 * (img.nnodes - 1) and img.nnodes <= vt.capacity(img.k, img.L)
        if name in SHAPES:
            assert (img.max_children, per_level, img.nwords) == SHAPES[name]
        if name in ("wide_32", "wide_33"):
            n = 32 if name == "wide_32" else 33
            assert (img.k, img.L) == (20, 3) and len(img.children[0]) == n == img.max_children
            assert sorted(len(img.children[c]) for c in img.children[0]) == list(range(1, n + 1))
            assert per_level == [0, n * (n + 1) // 2, 0]
        if name == "ragged":
            assert (img.k, img.L, img.max_children) == (10, 4, 10) and 300 <= img.nnodes <= 3000
            assert all(c > 0 for c in per_level) and set(counts[~img.is_leaf]) == set(range(1, 11))
            a, depth = img.children[0][0], 1  # the chain of single-child nodes under the root's first child
            while len(img.children[a]) == 1:
                a, depth = img.children[a][0], depth + 1
            assert depth == 4 and img.is_leaf[a]
            assert len(img.children[0]) == 10 and not img.is_leaf[img.children[0][9]]
            stopped = img.is_leaf & ~(img.weight > 0)
            assert 0.12 <= stopped.sum() / img.nwords <= 0.28
            assert all(stopped[img.level == lv].any() and (img.is_leaf & ~stopped)[img.level == lv].any() for lv in (1, 2, 3, 4))
            assert img.is_leaf[img.children[0][1]] and stopped[img.children[0][2]]
        if name == "ties_wide":
            for c in img.children:
                if c:
                    assert np.array_equal(img.desc[c[3]], img.desc[c[19]]) and np.array_equal(img.desc[c[15]], img.desc[c[16]])
        if name == "complement":
            assert (img.desc[1:] == ~vt.COMPLEMENT_QUERY).all() and np.array_equal(vt.queries(name)[0], vt.COMPLEMENT_QUERY)
    # the three orders: bfs is the identity numbering of a level-by-level tree, dfs keeps siblings contiguous but is not
    # level by level, scattered breaks sibling runs apart
    bfs, dfs, sc = imgs
    assert (np.diff(bfs.level) >= 0).all()
    assert all(c == list(range(c[0], c[0] + len(c))) for c in dfs.children if c)
    if name != "complement":
        assert any(c != list(range(c[0], c[0] + len(c))) for c in sc.children if len(c) > 1)
        assert not np.array_equal(sc.abstract, bfs.abstract)
    # a tree of two levels is the same file depth-first and breadth-first; a deeper one is not
    assert np.array_equal(dfs.abstract, bfs.abstract) == (bfs.level.max() <= 2 or name == "complement")
    assert (np.diff(dfs.level) < 0).any() == (bfs.level.max() > 2 and name != "complement")
    assert len(t) == bfs.nnodes


def test_a_tree_larger_than_its_header_is_not_written():
    """Root of 32 children with 1..32 children each is 561 nodes; a header of k = 20, L = 2 stands for 421, where every
    loader stops reading.  Hence wide_32 / wide_33 carry L = 3."""
    t = vt.tree("wide_32")
    assert len(t) == 561 and vt.capacity(20, 2) == 421 and vt.capacity(20, 3) == 8421
    small = vt.Tree(20, 2)
    small.children, small.parent, small.level, small.desc, small.weight = t.children, t.parent, t.level, t.desc, t.weight
    with pytest.raises(ValueError):
        vt.write(small, "bfs")


@pytest.mark.parametrize("name", NAMES)
def test_the_three_orders_are_one_vocabulary(walked, name):
    """Per feature the same (leaf descriptor, weight) and the same chain of ancestors' descriptors whatever the file
    order: only the ids are permuted."""
    q = vt.queries(name)
    seen = []
    for order in vt.ORDERS:
        img = vt.image(name, order)
        ref = ol.OracleVocabulary(img.blob)
        out = ref.transform(q, 0)
        leaf = img.leaf_of_word[out["word"]]
        assert np.array_equal(out["weight"].view(np.uint64), img.weight[leaf].view(np.uint64))
        seen.append((img.abstract[leaf], img.desc[leaf], out["weight"], img.level[leaf]))
        ids = np.stack([out["word"], ref.transform(q, img.L - 2)["node"]])  # word ids and the node ids of level 2
        if order == "bfs":
            first_ids = ids
        elif name != "complement" and (order == "scattered" or img.level.max() > 2):
            # the ids themselves differ: a loader that assumed one numbering would be caught
            assert not np.array_equal(ids, first_ids)
    for other in seen[1:]:
        for a, b in zip(seen[0], other):
            assert np.array_equal(a, b)


def test_full_20_L3_has_2048_distinct_live_words():
    img = vt.image("full_20_L3", "bfs")
    out = ol.OracleVocabulary(img.blob).transform(vt.queries("full_20_L3"), 0)
    assert len(np.unique(out["word"][out["weight"] > 0])) >= 2048
