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
