"""The tile-edge scene of the caller-bits SearchForTriangulation walk (tests/triangulation_edges.py) against the CPU oracle
alone: the node sizes are the ones promised, and every leg has the matches the GPU test relies on (tests/test_gpu_match.py)."""
import numpy as np
import pytest

import oracle_lib as ol
import triangulation_edges as te


def oracle(s, pattern, flags):
    ok, off = te.pair_bits(pattern)
    e1, e2 = s["flags"][flags]
    return ol.search_for_triangulation(s["d1"], s["a1"], e1, s["fv1"], s["d2"], s["a2"], e2, s["fv2"], ok, off, True)


def test_the_scene_has_the_promised_nodes():
    s = te.scene()
    (ids1, off1, idx1), (ids2, off2, idx2) = s["fv1"], s["fv2"]
    shared = np.intersect1d(ids1, ids2)
    assert shared.tolist() == te.IDS and te.ONLY1[0] in ids1 and te.ONLY2[0] in ids2
    sizes = [(int(np.diff(off1)[np.searchsorted(ids1, i)]), int(np.diff(off2)[np.searchsorted(ids2, i)])) for i in shared]
    assert sizes == te.SIZES
    assert sorted(idx1.tolist()) == list(range(len(s["d1"]))) and sorted(idx2.tolist()) == list(range(len(s["d2"])))
    i1, early, late = s["tie"]
    assert (s["d2"][early] == s["d1"][i1]).all() and (s["d2"][late] == s["d1"][i1]).all()
    at = {int(j): p for p, j in enumerate(s["lists2"][te.TIE])}
    assert (at[early], at[late]) == (127, 128)
    for e1, e2 in s["flags"].values():
        assert e1[i1] and e2[early] and e2[late]


@pytest.mark.parametrize("flags", ["all_one", "every_third_zero"])
@pytest.mark.parametrize("pattern", te.PATTERNS)
def test_the_oracle_finds_what_the_gpu_test_relies_on(pattern, flags):
    s = te.scene()
    n, m12 = oracle(s, pattern, flags)
    assert n == (m12 >= 0).sum()
    te.check_counts(s, pattern, flags, n, m12)
    if pattern == "none":
        ones = oracle(s, "ones", flags)
        assert ones[0] == n and np.array_equal(ones[1], m12)
        assert n >= (300 if flags == "all_one" else 100)
