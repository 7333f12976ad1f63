"""The ordered walks in the form a workgroup runs (csrc/vsg_walks_dev.h: rounds to a fixed point, then last writer, rotation
filter and edge list) against their definition, walk::search_last / walk::search_local of csrc/vsg_walks.h, both built for
the host (tests/_walkcore).  Compared on every case: nmatches, train_match, train_blocked, the edge list and the number of
claims per rotation bin.  The serial definition alone says whether a case is what it is meant to be."""
import numpy as np
import pytest

import walk_cases as wc


@pytest.fixture(scope="module")
def random_results():
    return [wc.run(c) for c in wc.random_cases()]


def test_the_random_set_covers_overwrites_filter_drops_and_both_list_forms():
    """Conditions on the fixture, from the serial definition and the generator alone."""
    inline = overflow = 0
    for c in wc.random_cases():
        inline += bool(((c["cnt"] > 0) & (c["cnt"] <= wc.INLINE)).any())
        overflow += bool((c["cnt"] > wc.INLINE).any())
        assert 0 <= c["nq"] <= 300 and (c["cnt"] <= 40).all()
    assert inline >= 1000 and overflow >= 1000


def test_random_cases_equal_the_serial_walk(random_results):
    assert len(random_results) >= 2000
    overwrite = sum(1 for r, _ in random_results if r["overwrites"] > 0)
    dropped = sum(1 for r, _ in random_results if r["dropped"] > 0)
    assert overwrite >= 100 and dropped >= 100, (overwrite, dropped)
    bad = [(seed, wc.same(r, d)) for seed, (r, d) in enumerate(random_results) if wc.same(r, d)]
    assert not bad, bad[:10]
    assert max(d["rounds"] for _, d in random_results) > 3  # chains of claims occur: the loop is not a one-round affair


@pytest.mark.parametrize("name", sorted(wc.directed()))
def test_directed_case_equals_the_serial_walk(name):
    r, d = wc.run(wc.directed()[name])
    assert wc.same(r, d) == []


def test_no_queries_and_empty_lists_keep_the_callers_slots():
    for name in ("no_queries", "no_queries_local", "empty_lists", "empty_lists_local"):
        c = wc.directed()[name]
        r, d = wc.run(c)
        assert r["nmatches"] == 0 and d["nmatches"] == 0 and (d["tm"] == -1).all() and not d["tb"].any()
        want = np.flatnonzero(c["slots_in"] >= 0) if c["slots_in"] is not None else np.zeros(0, np.int64)
        assert d["edge_feat"].tolist() == want.tolist()
        assert d["rounds"] <= 1


@pytest.mark.parametrize("name", ["pile_up_64", "pile_up_64_local"])
def test_a_pile_up_of_64_queries_takes_more_than_32_rounds_and_finishes(name):
    r, d = wc.run(wc.directed()[name])
    assert r["tm"][:64].tolist() == list(range(64)) and r["nmatches"] == 64  # query k ends on feature k
    assert d["rounds"] > 32 and d["rounds"] <= 65
    assert wc.same(r, d) == []


def test_last_writer_and_count_rules():
    r, d = wc.run(wc.directed()["last_writer"])
    # feature 5: claimed by 0 and 1 (unobserved), then by 2 (observed, blocks); query 3 moves to feature 6
    assert r["nmatches"] == 4 and r["tm"][5] == 2 and r["tm"][6] == 3 and r["tb"][5] == 1 and r["tb"][6] == 1
    assert wc.same(r, d) == []


def test_a_feature_claimed_in_a_winning_and_a_losing_bin_ends_unmatched():
    r, d = wc.run(wc.directed()["win_and_lose"])
    assert r["overwrites"] == 1 and r["dropped"] == 1 and r["bins"][3] == 1 and r["bins"][0] == 13
    assert r["tm"][3] == -1 and r["tb"][3] == 0 and r["nmatches"] == 13
    assert wc.same(r, d) == []


def test_three_maxima_threshold_and_bin_wrap():
    r, d = wc.run(wc.directed()["one_maximum"])
    assert r["bins"][0] == 21 and r["bins"][3] == 2 and r["bins"][7] == 1 and r["dropped"] == 3 and r["nmatches"] == 21
    assert wc.same(r, d) == []
    r, d = wc.run(wc.directed()["bin_wrap"])
    assert r["bins"][0] == 21 and r["bins"][3] == 3 and r["bins"].sum() == 24 and r["dropped"] == 0
    assert wc.same(r, d) == []


def test_local_ratio_at_its_edge_and_a_blocked_second_best():
    r, d = wc.run(wc.directed()["ratio_edge"])
    assert r["tm"][1] == 0 and r["tm"][3] == -1 and r["tm"][5] == 2 and r["nmatches"] == 2
    assert wc.same(r, d) == []
    r, d = wc.run(wc.directed()["second_blocked"])
    assert r["nmatches"] == 2 and r["tm"][2] == 1
    assert wc.same(r, d) == []
    r, d = wc.run(wc.directed()["second_open"])
    assert r["nmatches"] == 1 and r["tm"][2] == -1
    assert wc.same(r, d) == []


def test_an_overflow_is_summed_over_every_long_list_and_nothing_is_walked():
    """The window kernel reserves a long list's segment with one atomic whether or not it fits: after an overflow the host
    must add EVERY long list's length to its copy of the counter, also of the segments that start behind the array's end."""
    cnt = np.array([20, 5, 30, 16, 17], np.int32)
    inline = np.arange(5) * wc.INLINE
    # room for 8 entries behind the 5 inline slots: the three long lists were given 80 + 0, 80 + 20, 80 + 50
    off = np.where(cnt > wc.INLINE, 80 + np.array([0, 0, 20, 0, 50]), inline)
    assert wc.overflow_status(off, cnt, 8) == (1, 67, 0)
    # with room for all of them the same lists are no overflow (67 entries behind the slots)
    flags, total, _ = wc.overflow_status(off, cnt, 67)
    assert flags & 1 == 0 and total == 67


# ---- the cases past one trip of the workgroup's loops and at the LDS cap (walk_cases.big_cases, directed_high, cap_cases):
# what makes each of them what it claims to be, from the serial definition, so that the GPU tests that walk them on the
# device (tests/test_gpu_track_walk.py) cannot quietly lose their point

def test_the_lds_restatement_follows_the_kernels_constants():
    from pathlib import Path
    csrc = Path(__file__).resolve().parent.parent / "visual_sgraphs_amd" / "csrc"
    track, dev = (csrc / "vsg_track.hip").read_text(), (csrc / "vsg_walks_dev.h").read_text()
    assert "kWalkThreads = 1024, kWalkWaves = kWalkThreads / 64, kWalkStaticLds = kWalkWaves * 4, kWalkLdsMax = 64 * 1024" in track
    assert "return ((size_t)2 * nf + nq + walkdev::kScratchInts) * 4 + (size_t)2 * nq + nf;" in track
    assert "walk_lds_bytes(nq, nf) + kWalkStaticLds > kWalkLdsMax" in track and "enum { kScratchInts = 40 };" in dev
    assert (wc.LANES, wc.LDS_STATIC, wc.LDS_MAX) == (1024, 1024 // 64 * 4, 64 * 1024)
    for name, (nq, nf) in wc.CAP_SHAPES.items():  # the largest accepted shapes: one query more is refused
        assert wc.lds_bytes(nq, nf) + wc.LDS_STATIC == 65534 and not wc.over_cap(nq, nf), name
        assert wc.lds_bytes(nq + 1, nf) + wc.LDS_STATIC == 65540 and wc.over_cap(nq + 1, nf), name
        assert wc.OVER_CAP_SHAPES["over_" + name] == (nq + 1, nf)
    assert {(c["nq"], c["nf"]) for c in wc.cap_cases().values()} == set(wc.CAP_SHAPES.values()) | set(wc.OVER_CAP_SHAPES.values())
    assert all(c["form"] == wc.LOCAL for c in wc.cap_cases().values())


@pytest.mark.parametrize("name", sorted(wc.big_cases()))
def test_big_cases_go_round_the_workgroups_loops_and_equal_the_serial_walk(name):
    c = wc.big_cases()[name]
    nq, nf = c["nq"], c["nf"]
    r, d = wc.run(c)
    print(f"{name}: overwrites {r['overwrites']} dropped {r['dropped']} rounds {d['rounds']} edges {r['n_edges']} "
          f"edges >= 1024: {int((r['edge_feat'] >= wc.LANES).sum())} nmatches {r['nmatches']}")
    assert wc.same(r, d) == []
    assert (nq, nf) in wc.BIG_SHAPES and nq > wc.LANES and (c["cnt"] <= 40).all() and (c["cnt"] > wc.INLINE).any()
    assert r["n_edges"] > 0 and r["edge_feat"][-1] == nf - 1 and r["tm"][nf - 1] == -1 and r["tb"][nf - 1] == 1
    assert d["rounds"] >= 3
    if nf == 2049:
        assert int((r["edge_feat"] >= wc.LANES).sum()) >= 500 and int((r["tm"] >= wc.LANES).sum()) >= 1
    if c["form"] == wc.LAST:
        assert r["overwrites"] >= 100 and r["dropped"] >= 100


@pytest.mark.parametrize("name", ["pile_up_high", "pile_up_high_local"])
def test_a_pile_up_behind_1024_empty_lists_takes_more_than_32_rounds_and_finishes(name):
    c = wc.directed_high()[name]
    r, d = wc.run(c)
    assert c["nq"] == 1088 and (c["cnt"][:1024] == 0).all() and (c["cnt"][1024:] == 70).all()
    assert r["tm"][:64].tolist() == list(range(1024, 1088)) and r["nmatches"] == 64  # query 1024 + k ends on feature k
    assert 32 < d["rounds"] <= c["nq"] + 1
    assert wc.same(r, d) == []


@pytest.mark.parametrize("nf", [50, 2049])
def test_from_slots_blocks_features_by_their_entry_slots_alone(nf):
    c = wc.directed_high()["from_slots_%d" % nf]
    assert c["form"] == wc.LOCAL and c["blocked"] is None and c["nf"] == nf and len(c["slot_observed"]) == wc.N_STORE
    assert 0.4 < c["slot_observed"].mean() < 0.6
    blocked = wc.blocked_from_slots(c)
    r, d = wc.reference(c)
    assert wc.same(r, d) == [] and r["tb"][blocked != 0].all() and not (blocked.astype(bool) & (r["tm"] >= 0)).any()
    blocked_best = 0  # how often a feature blocked by the rule is the nearest candidate of a valid query
    for q in np.flatnonzero((c["q_valid"] != 0) & (c["cnt"] > 0)):
        l = c["ent"][c["off"][q]:c["off"][q] + c["cnt"][q]].astype(np.int64)
        blocked_best += int(blocked[(l & 0x7FFF)[np.argmin((l >> 15) & 0x1FF)]])
    print(f"from_slots_{nf}: blocked {int(blocked.sum())} blocked-best {blocked_best} rounds {d['rounds']} "
          f"edges {r['n_edges']} nmatches {r['nmatches']}")
    assert int(blocked.sum()) >= 10 and blocked_best >= 1
    if nf > wc.LANES:
        assert int(blocked[wc.LANES:].sum()) >= 10 and int((r["edge_feat"] >= wc.LANES).sum()) >= 100
    # without the rule the walk ends differently: the case depends on it
    r0, _ = wc.run(c)
    assert r0["tm"].tobytes() != r["tm"].tobytes()


def test_few_matches_and_few_edges_sit_on_both_sides_of_their_thresholds():
    D = wc.directed_high()
    for name, nm, flags in (("few_matches_19", 19, wc.ST_FEW_MATCHES), ("few_matches_20", 20, 0),
                            ("few_edges_2", 2, wc.ST_FEW_EDGES), ("few_edges_3", 3, 0)):
        c = D[name]
        r, d = wc.run(c)
        assert wc.same(r, d) == [] and r["nmatches"] == nm and r["n_edges"] == nm, name
        assert r["tm"][:nm].tolist() == list(range(nm)) and wc.status_flags(r, c) == flags, name
        assert d["flags"] == flags & wc.ST_FEW_EDGES, name  # the host build runs with min_matches = 0
    assert D["few_matches_19"]["min_matches"] == 20 == D["few_matches_20"]["min_matches"]


@pytest.mark.parametrize("name", sorted(wc.CAP_SHAPES))
def test_the_largest_accepted_shapes_equal_the_serial_walk(name):
    c = wc.cap_cases()[name]
    r, d = wc.run(c)
    print(f"{name}: rounds {d['rounds']} edges {r['n_edges']} edges >= 1024: {int((r['edge_feat'] >= wc.LANES).sum())} "
          f"nmatches {r['nmatches']}")
    assert wc.same(r, d) == [] and (c["nq"], c["nf"]) == wc.CAP_SHAPES[name]
    assert r["edge_feat"][-1] == c["nf"] - 1 and int((r["edge_feat"] >= wc.LANES).sum()) >= 500 and r["nmatches"] >= 100
    if c["nq"] > wc.LANES:  # (385 queries on 7000 features hardly collide)
        assert d["rounds"] >= 3 and int((r["tm"] >= wc.LANES).sum()) >= 100


def test_the_first_400_random_cases_cover_what_the_device_run_needs(random_results):
    """tests/test_gpu_track_walk.py walks seeds 0 .. 399 on the device."""
    res, cases = random_results[:400], wc.random_cases()[:400]
    overwrite = sum(1 for r, _ in res if r["overwrites"] > 0)
    dropped = sum(1 for r, _ in res if r["dropped"] > 0)
    long_walks = sum(1 for _, d in res if d["rounds"] > 3)
    inline = sum(1 for c in cases if ((c["cnt"] > 0) & (c["cnt"] <= wc.INLINE)).any())
    overflow = sum(1 for c in cases if (c["cnt"] > wc.INLINE).any())
    print(f"overwrite {overwrite} dropped {dropped} rounds > 3: {long_walks} inline {inline} overflow {overflow}")
    assert min(overwrite, dropped, long_walks, inline, overflow) >= 100
