"""The scenes of tests/match_scenes.py, proven on the CPU: every block's by-construction expectation is what the plain
restatement and the CPU oracle compute, and the directed positions cover the seams of the kernel's layout they are said
to cover.  The last part is what keeps tests/test_gpu_match_batched.py honest if the position list is ever edited."""
import itertools

import numpy as np
import pytest

import match_scenes as ms
import oracle_lib as ol


@pytest.mark.parametrize("which", list(ms.CASE_LISTS))
def test_every_block_gives_what_it_was_built_to_give(which):
    make, max_rows = ms.CASE_LISTS[which]
    cases = make()
    assert len({c["name"] for c in cases}) == len(cases) > 0
    a, b, na, nb = ms.pack_cases(cases, max_rows)
    ob, os_, oa = ol.block_best2_batch(a, na, b, nb)
    for i, c in enumerate(cases):
        assert 1 <= c["na"] <= max_rows and 1 <= c["nb"] <= max_rows, c["name"]
        (row, expect), = c["expect"].items()
        assert row == c["na"] - 1
        assert expect == c["stated"], c["name"]  # the chosen distances give what the case list states
        rb, rs, ra = ms.best2_reference(c["a"], c["na"], c["b"], c["nb"])
        assert (int(rb[row]), int(rs[row]), int(ra[row])) == expect, c["name"]
        # every row of the block, the random ones in front of the query included: restatement == oracle
        n = c["na"]
        assert np.array_equal(ob[i, :n], rb) and np.array_equal(os_[i, :n], rs) and np.array_equal(oa[i, :n], ra), c["name"]
        # the placed rows are at exactly the chosen distances from the query
        x = ms.unpack(c["a"][row])
        for r, d in c["placed"].items():
            assert int((x != ms.unpack(c["b"][r])).sum()) == d, (c["name"], r)


def test_the_case_lists_hold_what_the_plan_says():
    pairs = list(itertools.combinations(ms.P, 2))
    ties = ms.tie_cases()
    assert len(ties) == 3 * len(pairs) + len(ms.TRIPLES) == 3 * 136 + 6
    for kind in ("tie", "second before best", "second after best"):
        got = {(c["name"].split(" p=")[1]) for c in ties if c["name"].startswith(kind + " p=")}
        assert len(got) == len(pairs), kind
    assert {c["stated"][0] for c in ties} == set(ms.D_CYCLE)
    assert len(ms.placement_cases()) == 3 * 10 and {c["na"] - 1 for c in ms.placement_cases()} == set(ms.PLACEMENT_ROWS)
    assert len(ms.wide_cases()) == 6 and all(c["nb"] == 544 for c in ms.wide_cases())
    assert [c["stated"] for c in ms.extreme_cases()][:2] == [(256, 256, -1), (255, 256, 0)]
    assert ms.extreme_cases()[-1]["stated"] == (0, 0, 0)


def test_the_layout_formula_is_a_bijection_on_a_tile():
    """row offset (g & 3) + 8 * (g >> 2) + 4 * h over h = 0, 1 and g = 0..15 is every row of a tile once, and layout() is
    its inverse."""
    seen = {}
    for h in range(2):
        for g in range(16):
            seen[(g & 3) + 8 * (g >> 2) + 4 * h] = (h, g)
    assert sorted(seen) == list(range(32))
    for row in range(0, 600):
        grp, tile, h, g = ms.layout(row)
        assert seen[row % 32] == (h, g) and tile == row // 32 and grp == row // 256


def test_the_positions_cover_the_seams_they_claim():
    by_seam = {}
    for p, q in itertools.combinations(ms.P, 2):
        for s in ms.seams(p, q, ms.SEAM_NB):
            by_seam.setdefault(s, []).append((p, q))
    for s in ("same_lane", "other_half", "adjacent_tiles", "adjacent_groups", "full_vs_tail", "both_in_tail"):
        assert by_seam.get(s), s
    # first and last register of a lane, in both halves, and the same register of the two halves
    regs = {ms.layout(p)[2:] for p in ms.P if p < 32}
    assert {(0, 0), (0, 15), (1, 0), (1, 15)} <= regs
    # the tail tile of the seam blocks is partial, the wide block crosses the SECOND group edge on full tiles only
    assert ms.SEAM_NB % 32 and ms.SEAM_NB // 32 == ms.layout(288)[1] and ms.layout(256)[0] == 1
    assert ms.WIDE_NB % 32 == 0
    for p, q in ms.WIDE_PAIRS:
        assert ms.layout(q)[0] == 2 and ms.layout(p)[0] < 2 and "full_vs_tail" not in ms.seams(p, q, ms.WIDE_NB)
    assert "adjacent_groups" in ms.seams(511, 512, ms.WIDE_NB) and "distant_groups" in ms.seams(255, 512, ms.WIDE_NB)
    # the placement pairs: one inside a tile across the halves, one across a group edge, one full tile against the tail
    assert [ms.seams(p, q, ms.SEAM_NB) for p, q in ms.PLACEMENT_PAIRS] == [
        ["other_half"], ["adjacent_groups", "adjacent_tiles"], ["adjacent_tiles", "full_vs_tail"]]
    # query rows: every wave of the first x-workgroup, both query sets u of a wave, first and last column of a set, and
    # the second x-workgroup
    where = {(r // ms.WG_ROWS, (r % ms.WG_ROWS) // 64, (r % 64) // 32, r % 32) for r in ms.PLACEMENT_ROWS}
    assert {(wg, w) for wg, w, _, _ in where} >= {(0, 0), (0, 1), (0, 2), (0, 3), (1, 0)}
    assert {(wg, u) for wg, _, u, _ in where} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {c for _, _, _, c in where} == {0, 31}


def test_the_count_scene_is_what_the_plan_says_and_the_oracle_agrees():
    a, b, na, nb = ms.count_scene()
    M = ms.COUNT_MAX_ROWS
    pairs = list(zip(na.tolist(), nb.tolist()))
    assert a.shape == b.shape == (len(pairs), M, 32) and M == 320
    for p in [(0, 300), (300, 0), (0, 0), (1, 1), (1, 320), (320, 1), (320, 320), (321, 289), (400, 289),
              (2 ** 31 - 1, 289), (65, 321), (65, 400), (65, 2 ** 31 - 1), (-1, 289), (65, -1)]:
        assert p in pairs, p
    assert {n for n, m in pairs if m == 289} >= {31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257}
    assert {m for n, m in pairs if n == 65} >= {31, 32, 33, 255, 256, 257, 287, 288, 289}
    # an empty block sits next to a full one
    assert any(ms.clamp(pairs[i][0], M) == 0 and ms.clamp(pairs[i + 1][0], M) >= 256 or
               ms.clamp(pairs[i + 1][0], M) == 0 and ms.clamp(pairs[i][0], M) >= 256 for i in range(len(pairs) - 1))
    inside = [i for i, (n, m) in enumerate(pairs) if 0 <= n <= M and 0 <= m <= M]
    ob, os_, oa = ol.block_best2_batch(a[inside], na[inside], b[inside], nb[inside])
    ties = 0
    for k, i in enumerate(inside):
        rb, rs, ra = ms.best2_reference(a[i], na[i], b[i], nb[i])
        n = int(na[i])
        assert np.array_equal(ob[k, :n], rb) and np.array_equal(os_[k, :n], rs) and np.array_equal(oa[k, :n], ra), pairs[i]
        ties += int((rb == rs).sum())
    assert ties > 500  # tie-heavy: second == best is common, not an accident


def test_the_restatement_on_its_own_edges():
    z, o = np.zeros((3, 32), np.uint8), np.full((3, 32), 255, np.uint8)
    for nb in (0, -1):
        assert [v.tolist() for v in ms.best2_reference(z, 2, z, nb)] == [[256, 256], [256, 256], [-1, -1]]
    assert [v.tolist() for v in ms.best2_reference(z, 1, o, 3)] == [[256], [256], [-1]]
    assert [v.tolist() for v in ms.best2_reference(z, 1, z, 1)] == [[0], [256], [0]]
    assert [v.tolist() for v in ms.best2_reference(z, 1, z, 3)] == [[0], [0], [0]]
    assert all(len(v) == 0 for v in ms.best2_reference(z, -1, z, 3))
    assert ms.scan_distances([]) == (256, 256, -1) and ms.scan_distances([256, 256]) == (256, 256, -1)
    assert ms.scan_distances([7, 5, 5, 9]) == (5, 5, 1) and ms.scan_distances([5, 256]) == (5, 256, 0)


def test_stale_rows_are_copies_of_the_queries_and_leave_the_counted_rows_alone():
    a, b, na, nb = ms.count_scene()
    M = ms.COUNT_MAX_ROWS
    sa, sb = ms.with_stale_rows(a, b, na, nb, M)
    hit = 0
    for i in range(len(a)):
        n, m = ms.clamp(na[i], M), ms.clamp(nb[i], M)
        assert np.array_equal(sa[i, :n], a[i, :n]) and np.array_equal(sb[i, :m], b[i, :m])
        if n and m < M:
            assert np.array_equal(sb[i, m], a[i, 0])  # the first stale row, in the partial tail tile where there is one
            # reading the stale rows WOULD change the answer
            hit += int(not np.array_equal(ms.best2_reference(sa[i], n, sb[i], M)[2], ms.best2_reference(a[i], n, b[i], m)[2]))
    assert hit >= 20
