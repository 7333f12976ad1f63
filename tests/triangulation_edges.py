"""A directed scene for the tile edges of the SearchForTriangulation walk (k_triangulation_walk: KF1 rows in chunks of 128, KF2
rows in tiles of 128) with the predicate as caller-made bits, built on the CPU so that tests/test_triangulation_edges.py can
check it with the oracle alone before the GPU test (tests/test_gpu_match.py) uses it:

  * shared vocabulary nodes of (KF1 rows, KF2 rows) = SIZES, one node only KF1 has and one only KF2 has, the features of a
    node scattered over the frame (FeatureVectors from the builder of tests/epipolar_scenes.py);
  * KF2 row j of a node is a copy of KF1 row j % na of the node with 0..5 bits flipped, every other pair of descriptors is
    random (distance ~128), so the candidates of a KF1 row are its own copies and equal distances are common;
  * in the (129, 129) node the KF2 rows at positions 127 and 128 are EXACT copies of KF1 row 127: the later of the two equal
    distances lies in the second tile;
  * four bit patterns and two settings of the eligibility flags (all one; every third feature zero -- the features the
    single-row nodes and the tie depend on have indices that are no multiple of 3)."""
import functools

import numpy as np

import epipolar_scenes as es

SIZES = [(1, 1), (1, 129), (129, 1), (128, 128), (129, 129), (257, 130)]
IDS = [4, 9, 15, 22, 31, 47]
ONLY1, ONLY2 = (12, 7), (50, 5)   # (node id, rows) of the nodes one side has
PATTERNS = ("none", "ones", "zeros", "last_bit_of_every_node")
TIE = 4                           # the (129, 129) node


def _scatter(n, keep, rng):
    """A permutation of range(n) whose entries at the positions `keep` are no multiple of 3."""
    perm = rng.permutation(n)
    free = [q for q in range(n) if q not in keep and perm[q] % 3]
    for p in keep:
        if perm[p] % 3 == 0:
            q = free.pop()
            perm[p], perm[q] = perm[q], perm[p]
    return perm


@functools.lru_cache(maxsize=None)
def scene(seed=5):
    rng = np.random.default_rng(seed)
    sa, sb = [a for a, _ in SIZES], [b for _, b in SIZES]
    n1, n2 = sum(sa) + ONLY1[1], sum(sb) + ONLY2[1]
    at1, at2 = np.concatenate([[0], np.cumsum(sa)]), np.concatenate([[0], np.cumsum(sb)])
    lists1 = es._node_lists(_scatter(n1, {at1[1], at1[2], at1[TIE] + 127}, rng), sa + [ONLY1[1]])
    lists2 = es._node_lists(_scatter(n2, {at2[2], at2[TIE] + 127, at2[TIE] + 128}, rng), sb + [ONLY2[1]])
    d1 = rng.integers(0, 256, (n1, 32)).astype(np.uint8)
    d2 = rng.integers(0, 256, (n2, 32)).astype(np.uint8)
    a1 = rng.uniform(0, 360, n1).astype(np.float32)
    a2 = rng.uniform(0, 360, n2).astype(np.float32)
    for s, (a, b) in enumerate(SIZES):
        for j in range(b):
            src, dst = lists1[s][j % a], lists2[s][j]
            d2[dst], a2[dst] = d1[src], a1[src]
            for bit in rng.integers(0, 256, rng.integers(0, 6)):
                d2[dst, bit >> 3] ^= np.uint8(1 << (bit & 7))
    l1, l2 = lists1[TIE], lists2[TIE]
    d2[l2[127]] = d2[l2[128]] = d1[l1[127]]
    a2[l2[127]] = a2[l2[128]] = a1[l1[127]]
    nodes1 = dict(zip(IDS + [ONLY1[0]], lists1))
    nodes2 = dict(zip(IDS + [ONLY2[0]], lists2))
    third1, third2 = np.ones(n1, np.uint8), np.ones(n2, np.uint8)
    third1[::3] = 0
    third2[::3] = 0
    return dict(d1=d1, a1=a1, d2=d2, a2=a2, fv1=es._fv(nodes1), fv2=es._fv(nodes2), lists1=lists1[:-1], lists2=lists2[:-1],
                flags={"all_one": (np.ones(n1, np.uint8), np.ones(n2, np.uint8)), "every_third_zero": (third1, third2)},
                tie=(int(l1[127]), int(l2[127]), int(l2[128])))


def keypoints(angle, dtype):
    """Keypoints with these angles somewhere in a 640 x 480 image, octave 0 (what a resident frame needs besides descriptors)."""
    k = np.zeros(len(angle), dtype)
    k["x"], k["y"] = np.linspace(1, 638, len(angle)), np.linspace(1, 478, len(angle))
    k["angle"], k["size"] = angle, 31.0
    return k


def pair_bits(pattern):
    """(pair_ok words, pair_off) of the pattern in the layout of vsg_search_for_triangulation -- the shared nodes in ascending
    id are SIZES in order -- or (None, None)."""
    if pattern == "none":
        return None, None
    pair_off = np.concatenate([[0], np.cumsum([a * b for a, b in SIZES])]).astype(np.int32)
    nwords = (int(pair_off[-1]) + 31) // 32
    if pattern == "ones":
        return np.full(nwords, 0xFFFFFFFF, np.uint32), pair_off
    words = np.zeros(nwords, np.uint32)
    if pattern == "last_bit_of_every_node":
        for last in pair_off[1:] - 1:
            words[last >> 5] |= np.uint32(1 << (int(last) & 31))
    return words, pair_off


def check_counts(s, pattern, flags, n, matches12):
    """What the scene promises of the oracle's result (and so of the kernel's)."""
    if pattern == "zeros":
        assert n == 0 and (matches12 == -1).all()
    if pattern in ("none", "ones"):
        for (a, b), rows in zip(SIZES, s["lists1"]):
            if a * b > 1:
                assert (matches12[rows] >= 0).any(), (a, b)
        i1, early, late = s["tie"]
        assert matches12[i1] == late != early   # the later of the equal distances, across the tile edge
    if pattern == "last_bit_of_every_node":
        last = [rows[-1] for rows in s["lists1"]]
        assert set(np.flatnonzero(matches12 >= 0)) <= set(last)
