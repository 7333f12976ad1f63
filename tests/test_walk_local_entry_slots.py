"""The rule vsg_frame_track_local_map's walk kernel implements for features that hold a map point on entry, on the host
build of the walks (tests/_walkcore, as it is): a feature is blocked on entry iff it has a slot whose point is observed
(ORBmatcher.cc:86-88).  The local round form (csrc/vsg_walks_dev.h) with the features' entry slots and the blocked array
computed from them must equal walk::search_local given the same blocked array plus the caller's slot loop: per feature the
claimant's slot, or else the entry slot; an unobserved entry point can be overwritten (:130), an observed one blocks."""
import numpy as np
import pytest

import walk_cases as wc

I32 = np.int32
N_STORE = 5000


def blocked_from(slots_in, store_observed):
    """what k_track_walk's prologue derives: slots_in >= 0 and observed[slot]"""
    return (slots_in >= 0) & (store_observed[np.maximum(slots_in, 0)] != 0)


def local_case(lists, nf, slots_in, store_observed, q_slot, q_valid=None, nnratio=0.8, rng=None):
    slots_in, q_slot = np.asarray(slots_in, I32), np.asarray(q_slot, I32)
    return wc.case(wc.LOCAL, lists, nf, observed=store_observed[q_slot] != 0, blocked=blocked_from(slots_in, store_observed),
                   q_slot=q_slot, slots_in=slots_in, q_valid=q_valid, check=0, nnratio=nnratio, rng=rng)


def random_case(seed):
    rng = np.random.default_rng(10_000 + seed)
    nq, nf = int(rng.integers(0, 301)), int(rng.integers(41, 401))
    store_observed = (rng.random(N_STORE) < rng.choice([0.0, 0.5, 0.9, 1.0])).astype(np.uint8)
    spread, n_centres = int(rng.choice([41, 60, 120])), int(rng.choice([1, 3, 20, 200]))
    centres = rng.integers(0, nf, n_centres)
    lists = []
    for q in range(nq):
        n = int(rng.integers(0, 41)) if rng.random() > 0.15 else 0
        idx = (centres[rng.integers(0, n_centres)] + rng.permutation(spread)[:n]) % nf
        lists.append(wc.entry(idx, rng.choice(wc.DISTS, n), rng.integers(0, 3, n)))
    slots_in = np.where(rng.random(nf) < rng.choice([0.1, 0.3, 0.7]), rng.integers(0, N_STORE, nf), -1)
    return local_case(lists, nf, slots_in, store_observed, rng.integers(0, N_STORE, nq),
                      q_valid=None if rng.random() < 0.5 else rng.random(nq) < 0.9,
                      nnratio=float(rng.choice([0.6, 0.8, 1.0])), rng=rng)


def outcome(c):
    """the slot every feature ends with, from the edge list"""
    r, d = wc.run(c)
    assert wc.same(r, d) == []
    fs = np.full(c["nf"], -1, I32)
    fs[d["edge_feat"]] = d["edge_slot"]
    return r, d, fs


def test_500_random_cases_equal_the_serial_walk_and_the_slot_loop():
    overwritten = blocked_best = kept = 0
    for seed in range(500):
        c = random_case(seed)
        r, d, fs = outcome(c)
        si, tm = c["slots_in"], r["tm"]
        qs = np.append(c["q_slot"], -1)  # (never read through tm when there is no query)
        want = np.where(tm >= 0, qs[np.maximum(tm, 0)], si).astype(I32)  # the caller's loop, restated
        assert fs.tobytes() == np.where(want >= 0, want, -1).astype(I32).tobytes(), seed
        assert not (c["blocked"].astype(bool) & (tm >= 0)).any(), seed  # a feature blocked on entry is never claimed
        overwritten += int(((si >= 0) & (tm >= 0)).sum())
        kept += int(((si >= 0) & (tm < 0)).sum())
        for q in range(c["nq"]):  # how often a feature blocked on entry is the nearest candidate of a query
            l = c["ent"][c["off"][q]:c["off"][q] + c["cnt"][q]].astype(np.int64)
            if len(l):
                blocked_best += int(c["blocked"][(l & 0x7FFF)[np.argmin((l >> 15) & 0x1FF)]])
    # conditions on the fixture: every branch of the rule occurs often
    assert overwritten >= 100 and kept >= 1000 and blocked_best >= 100, (overwritten, kept, blocked_best)


def directed():
    obs = np.zeros(N_STORE, np.uint8)
    obs[[10, 11, 12, 13]] = 1  # observed points; 20 .. 29 are not
    D = {}
    # feature 3 holds the unobserved point 20; query 0 (point 10) takes it
    D["unobserved_entry_slot_is_overwritten"] = local_case(
        [wc.entry([3, 4], [20, 90], [1, 2])], 8, [-1, -1, -1, 20, -1, -1, -1, -1], obs, [10])
    # feature 3 holds the observed point 12 and is the best candidate of both queries: both move to their second
    # candidates (5 and 6), feature 3 keeps its point
    D["observed_entry_slot_is_best_of_two_queries"] = local_case(
        [wc.entry([3, 5], [10, 40], [1, 2]), wc.entry([3, 6], [15, 45], [1, 2])], 8, [-1, -1, -1, 12, -1, -1, -1, -1], obs,
        [10, 21])
    # feature 7 holds a point and no list names it: it stays an edge with its entry slot
    D["entry_slot_on_a_feature_no_list_names"] = local_case(
        [wc.entry([1], [30]), wc.entry([2], [30])], 8, [-1, -1, -1, -1, -1, -1, -1, 25], obs, [10, 11])
    return D


@pytest.mark.parametrize("name", sorted(directed()))
def test_directed_case(name):
    c = directed()[name]
    r, d, fs = outcome(c)
    if name == "unobserved_entry_slot_is_overwritten":
        assert not c["blocked"].any() and r["tm"].tolist() == [-1, -1, -1, 0, -1, -1, -1, -1]
        assert fs.tolist() == [-1, -1, -1, 10, -1, -1, -1, -1] and r["nmatches"] == 1
    elif name == "observed_entry_slot_is_best_of_two_queries":
        assert c["blocked"].tolist() == [0, 0, 0, 1, 0, 0, 0, 0]
        assert r["tm"].tolist() == [-1, -1, -1, -1, -1, 0, 1, -1] and r["nmatches"] == 2
        assert fs.tolist() == [-1, -1, -1, 12, -1, 10, 21, -1]
        assert d["edge_feat"].tolist() == [3, 5, 6]
    else:
        assert r["tm"].tolist() == [-1, 0, 1, -1, -1, -1, -1, -1] and fs.tolist() == [-1, 10, 11, -1, -1, -1, -1, 25]
        assert d["edge_feat"].tolist() == [1, 2, 7] and d["edge_slot"].tolist() == [10, 11, 25]
