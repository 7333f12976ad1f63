"""GPU tests of k_track_walk ALONE (vsg_debug_track_walk of include/vsg_orb_debug.h: the ordered walk of the two chain
calls, launched through their own launch function) against the serial definition, walk::search_last / walk::search_local of
csrc/vsg_walks.h built for the host (the `ref` side of walk_cases.run).  What the workgroup adds to the round form the host
build replays serially -- 1024 lanes going round their stride, LDS atomics, barriers between the phases, the ballot
compaction's running base, the byte arrays behind the int arrays in LDS, the prologue that derives "blocked on entry" -- is
what these cases are for: directed lists, 400 random cases, shapes past 1024 features and queries, and the two largest
shapes the LDS cap accepts.  Every output is an integer and is compared whole, bit for bit; the rounds are deterministic
(each round's choices read only the claims of the round before) and equal the host round form's.  What makes each case
what it claims to be is asserted without a GPU in tests/test_walk_rounds.py."""
import functools
import time

import numpy as np
import pytest

import walk_cases as wc
from visual_sgraphs_amd import orb

pytestmark = pytest.mark.gpu
I32, U8 = np.int32, np.uint8
S32, S8 = orb.WALK_SENTINEL_I32, orb.WALK_SENTINEL_U8
INVALID, CAPACITY = -6, -2


@functools.lru_cache(maxsize=None)
def named():
    """every case with a name, old and new; nobody writes to a case"""
    return {**wc.directed(), **wc.directed_high(), **wc.big_cases(), **wc.cap_cases()}


def untouched(o):
    return all((o[k] == S32).all() for k in ("tm", "feat_slots", "edges_feat", "edges_slot")) and \
        all((o[k] == S8).all() for k in ("tb", "feat_observed"))


def walk(c, cap=None):
    return orb.debug_track_walk(c, cap=cap, min_matches=c.get("min_matches", 0), slot_observed=c.get("slot_observed"))


def check(c, label):
    """the device walk of one case against the definition; -> (device, ref, host round form)"""
    r, d = wc.reference(c)
    t0 = time.perf_counter()
    g = walk(c)
    ms = (time.perf_counter() - t0) * 1e3
    print(f"{label}: nq {c['nq']} nf {c['nf']} nmatches {g['nmatches']} edges {g['n_edges']} rounds {g['rounds']} "
          f"flags {g['flags']} call {ms:.2f} ms")
    assert (g["nmatches"], g["n_edges"]) == (r["nmatches"], r["n_edges"]), label
    for k in ("tm", "tb", "edge_feat", "edge_slot", "bins"):
        assert g[k].dtype == r[k].dtype and g[k].tobytes() == r[k].tobytes(), (label, k)
    # the edge arrays behind the list are nobody's: still the sentinel
    assert (g["edges_feat"][g["n_edges"]:] == S32).all() and (g["edges_slot"][g["n_edges"]:] == S32).all(), label
    fs = wc.feat_slots_of(r, c)
    assert g["feat_slots"].tobytes() == fs.tobytes(), label
    table = c.get("slot_observed")
    want_fo = np.full(c["nf"], S8, U8) if table is None else np.where(fs >= 0, table[np.maximum(fs, 0)], 0).astype(U8)
    assert g["feat_observed"].tobytes() == want_fo.tobytes(), label
    # the host round form: the same rounds, the same flags (it runs with min_matches = 0)
    assert g["rounds"] == d["rounds"] and g["flags"] == wc.status_flags(r, c), label
    assert g["flags"] & ~wc.ST_FEW_MATCHES == d["flags"], label
    assert g["overflow_sum"] == int(c["cnt"][c["cnt"] > wc.INLINE].sum()), label
    return g, r, d


@pytest.mark.parametrize("name", sorted(wc.directed()))
def test_directed_case_equals_the_serial_walk(name):
    g, _, _ = check(named()[name], name)
    if name.startswith("pile_up_64"):
        assert 32 < g["rounds"] <= 65


@pytest.mark.parametrize("name", sorted(wc.directed_high()))
def test_directed_case_past_one_trip_equals_the_serial_walk(name):
    c = named()[name]
    g, _, _ = check(c, name)
    if name.startswith("pile_up_high"):
        assert g["tm"][:64].tolist() == list(range(1024, 1088)) and 32 < g["rounds"] <= c["nq"] + 1
    if name.startswith("few_"):
        want = {"few_matches_19": wc.ST_FEW_MATCHES, "few_matches_20": 0, "few_edges_2": wc.ST_FEW_EDGES, "few_edges_3": 0}
        assert g["flags"] == want[name]
    if name.startswith("from_slots"):  # nothing but the prologue's rule blocks a feature on entry here
        blocked = wc.blocked_from_slots(c)
        assert c["blocked"] is None and blocked.sum() >= 10 and g["tb"][blocked != 0].all()


def test_400_random_cases_equal_the_serial_walk():
    cases = wc.random_cases()[:400]
    refs = [wc.run(c) for c in cases]
    # conditions on the set, from the definition alone
    overwrite = sum(1 for r, _ in refs if r["overwrites"] > 0)
    dropped = sum(1 for r, _ in refs if r["dropped"] > 0)
    long_walks = sum(1 for _, d in refs if d["rounds"] > 3)
    inline = sum(1 for c in cases if ((c["cnt"] > 0) & (c["cnt"] <= wc.INLINE)).any())
    overflow = sum(1 for c in cases if (c["cnt"] > wc.INLINE).any())
    assert min(overwrite, dropped, long_walks, inline, overflow) >= 100, (overwrite, dropped, long_walks, inline, overflow)
    t0 = time.perf_counter()
    bad = []
    for seed, (c, (r, d)) in enumerate(zip(cases, refs)):
        g = walk(c)
        diff = [k for k in ("nmatches", "n_edges") if g[k] != r[k]]
        diff += [k for k in ("tm", "tb", "edge_feat", "edge_slot", "bins") if g[k].tobytes() != r[k].tobytes()]
        diff += ["feat_slots"] if g["feat_slots"].tobytes() != wc.feat_slots_of(r, c).tobytes() else []
        diff += ["feat_observed"] if not (g["feat_observed"] == S8).all() else []
        diff += ["edge tail"] if not (g["edges_feat"][g["n_edges"]:] == S32).all() else []
        diff += ["rounds"] if g["rounds"] != d["rounds"] else []
        diff += ["flags"] if g["flags"] != d["flags"] else []
        if diff:
            bad.append((seed, diff))
    print(f"400 device walks in {time.perf_counter() - t0:.2f} s")
    assert not bad, bad[:10]


@pytest.mark.parametrize("name", sorted(wc.big_cases()))
def test_big_case_equals_the_serial_walk(name):
    c = named()[name]
    g, r, _ = check(c, name)
    assert g["edge_feat"][-1] == c["nf"] - 1  # the last feature: the last lane of the last trip that has one
    if c["nf"] > wc.LANES:
        assert (g["edge_feat"] >= wc.LANES).any() and (g["tm"] >= wc.LANES).any()


def test_overflow_statuses_and_nothing_else_is_written():
    """The layouts of test_an_overflow_is_summed_over_every_long_list_and_nothing_is_walked, and a list that starts in
    front of the array."""
    cnt = np.array([20, 5, 30, 16, 17], I32)
    off = np.where(cnt > wc.INLINE, 80 + np.array([0, 0, 20, 0, 50]), np.arange(5) * wc.INLINE).astype(I32)
    before = off.copy()
    before[1] = -5

    def lists(off, cap, nf):
        n_ent = 5 * wc.INLINE + cap
        return dict(form=wc.LAST, nq=5, nf=nf, n_ent=n_ent, ent=np.zeros(n_ent, np.uint32), off=off, cnt=cnt, q_valid=None,
                    observed=np.ones(5, U8), blocked=None, q_angle=np.zeros(5, np.float32),
                    t_angle=np.zeros(max(nf, 1), np.float32), q_slot=np.arange(5, dtype=I32), slots_in=None, check=1,
                    nnratio=0.8)

    layouts = ((off, 8, 50, (1, 67, 0)), (off, 8, 0, (1, 67, 0)), (off, 67, 0, None), (before, 67, 50, None))
    for off_, cap, nf, want in layouts:
        g = walk(lists(off_, cap, nf), cap=cap)
        assert (g["flags"], g["overflow_sum"], g["nmatches"]) == wc.overflow_status(off_, cnt, cap), (cap, nf)
        if want is not None:
            assert (g["flags"], g["overflow_sum"], g["nmatches"]) == want
        if g["flags"] & wc.ST_OVERFLOW:
            assert untouched(g) and g["n_edges"] == 0 and g["rounds"] == 0 and not g["bins"].any(), (cap, nf)
    assert wc.overflow_status(off, cnt, 67)[0] & wc.ST_OVERFLOW == 0
    assert wc.overflow_status(before, cnt, 67)[0] & wc.ST_OVERFLOW
    check(named()["last_writer"], "after the overflows")


@pytest.mark.parametrize("name", sorted(wc.CAP_SHAPES))
def test_the_largest_accepted_shape_runs_and_one_query_more_is_refused(name):
    """65534 of the 65536 bytes of LDS the kernel allows itself, for a workgroup of 1024 lanes."""
    c = named()[name]
    assert wc.lds_bytes(c["nq"], c["nf"]) + wc.LDS_STATIC == 65534
    check(c, name)
    over = named()["over_" + name]
    assert (over["nq"], over["nf"]) == (c["nq"] + 1, c["nf"]) and wc.over_cap(over["nq"], over["nf"])
    with pytest.raises(orb.VsgError) as e:
        walk(over)
    assert e.value.code == CAPACITY and untouched(e.value.outputs) and (e.value.outputs["status"] == S32).all()
    check(named()["big_local_1500_1025"], "after the refusal")


def test_every_refusal_leaves_the_outputs_alone_and_the_thread_usable():
    lib = orb.load_library()
    c = named()["from_slots_50"]
    table, pos = c["slot_observed"], {k: i for i, k in enumerate(orb.WALK_ARGS)}

    def raw(case=c, table=table, **replace):
        args, out, keep = orb.debug_track_walk_args(case, slot_observed=table)
        for k, v in replace.items():
            args[pos[k]] = v
        rc = lib.vsg_debug_track_walk(*args)
        if rc < 0:  # an error writes nothing
            assert untouched(out) and (out["status"] == S32).all(), replace
        return rc

    def after(code, rc, what):
        assert rc == code, (what, rc, code)
        check(c, "after " + what)

    for k in ("ent", "off", "cnt", "q_angle", "t_angle", "train_match", "train_blocked", "feat_slots", "feat_observed",
              "edge_feat", "edge_slot", "status"):
        after(INVALID, raw(**{k: None}), "NULL " + k)
    for k in ("nq", "nf", "n_ent", "cap", "n_slots"):
        after(INVALID, raw(**{k: -1}), "negative " + k)
    after(INVALID, raw(nf=32769), "nf past the index field")
    for form in (-1, 2):
        after(INVALID, raw(form=form), "form %d" % form)
    for key, where in (("q_slot", 3), ("slots_in", int(np.flatnonzero(c["slots_in"] < 0)[0]))):
        for v in (-2, len(table)):
            a = c[key].copy()
            a[where] = v
            after(INVALID, raw(case=dict(c, **{key: a})), "%s[%d] = %d" % (key, where, v))
            # without the table nothing is indexed by a slot: such a call is taken
            assert raw(case=dict(c, **{key: a}), table=None) == 0
    after(CAPACITY, raw(case=named()["over_cap_features"], table=None), "one query too many")
    assert raw() == 0
