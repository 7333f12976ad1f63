"""The cases of the FeatureVector argument checks (visual_sgraphs_amd/csrc/vsg_fv.h), shared by tests/test_fv_args.py (the host
core loaded into Python) and tests/test_sanitizers_fv.py (the same core as a sanitized program)."""
import numpy as np

I32 = np.int32


def _a(*v):
    return np.asarray(v, I32).reshape(-1)


def fv_check_cases():
    """name -> (node_id, off, idx, n, null arrays?, expected)"""
    ids, off, idx = _a(3, 7, 12), _a(0, 2, 2, 5), _a(4, 0, 9, 1, 5)   # a node without features; features 0 and n - 1
    cases = {"valid": (ids, off, idx, 10, False, 1),
             "no_nodes_null_arrays": (_a(), _a(0), _a(), 10, True, 1),
             "no_nodes_no_features": (_a(), _a(0), _a(), 0, False, 1),
             "off0_is_1": (ids, _a(1, 2, 2, 5), idx, 10, False, 0),
             "descending_offset": (ids, _a(0, 3, 2, 5), idx, 10, False, 0),
             "equal_node_ids": (_a(3, 7, 7), off, idx, 10, False, 0),
             "descending_node_ids": (_a(3, 12, 7), off, idx, 10, False, 0)}
    for bad in (-1, 10, 1 << 30):
        b = idx.copy()
        b[3] = bad
        cases["idx_%d" % bad] = (ids, off, b, 10, False, 0)
    return cases


def id_sets(seed=7):
    """name -> (ascending ids of A, ascending ids of B)"""
    rng = np.random.default_rng(seed)
    pick = lambda k: np.sort(rng.choice(2000, k, replace=False)).astype(I32)
    same = pick(40)
    a300, b300 = pick(300), pick(300)
    assert 10 <= len(np.intersect1d(a300, b300)) < 300
    return {"disjoint": (_a(1, 5, 9, 13), _a(0, 2, 6, 20, 21)), "identical": (same, same.copy()),
            "a_empty": (_a(), pick(5)), "b_empty": (pick(5), _a()), "one_each_same": (_a(8), _a(8)),
            "one_each_different": (_a(8), _a(9)), "random_300": (a300, b300)}


def offsets(ids, seed):
    """Seeded CSR offsets of 0..3 features per node."""
    rng = np.random.default_rng(seed)
    return np.concatenate([[0], np.cumsum(rng.integers(0, 4, len(ids)))]).astype(I32)


def expected_join(idA, offA, idB, offB):
    """numpy.intersect1d on the ids: the shared nodes in ascending id with both sides' ranges."""
    _, ia, ib = np.intersect1d(idA, idB, return_indices=True)
    return np.stack([offA[ia], offA[ia + 1], offB[ib], offB[ib + 1]], 1).astype(I32).reshape(-1, 4)


def pair_bits_cases():
    """name -> (na, nb, pair_off, expected)"""
    na, nb = _a(3, 1, 129), _a(5, 7, 130)
    exact = np.concatenate([[0], np.cumsum(na.astype(np.int64) * nb)]).astype(I32)
    slack = exact.copy()
    slack[1:] += 11   # unused bits behind the first node
    slack[3:] += 64
    short = exact.copy()
    short[-1] -= 1
    shifted = exact - 1
    return {"exact": (na, nb, exact, 1), "slack": (na, nb, slack, 1), "one_bit_short_in_the_last_node": (na, nb, short, 0),
            "negative_first_offset": (na, nb, shifted, 0), "first_offset_not_zero": (na, nb, exact + 5, 1),
            "node_beyond_int32": (_a(50000), _a(50000), _a(0, 2**31 - 1), 0),
            # 50 000 x 50 000 = 2.5e9 bits; offsets whose int32 difference wraps to exactly that count are refused as well
            "node_beyond_int32_wrapped": (_a(50000), _a(50000), _a(2**31 - 1, int(np.int64(2**31 - 1 + 2500000000) - 2**32)), 0)}
