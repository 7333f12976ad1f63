"""The device-resident KeyFrameDatabase (vsg_kfdb_*) and vsg_vocab_score at their kernel edges, bit for bit against
tests/kfdb_reference.py: the directed scenes of tests/kfdb_scenes.py, BowVector lengths around the wavefront width, the
largest query (12288 words: 48 KB of dynamic LDS + 2 KB static), the second grid-stride pass (> 4096 items / candidates),
the one-thread-per-keyframe kernels at 255 / 256 / 257 / 513 keyframes with 64-bit ids, VSG_ERR_CAPACITY, every host-side
refusal, growth of the store, and the C++ adaptor.  Lists are compared id for id and, after every query, the six KeyFrame
members the queries read and write (tests/kfdb_both.py).  No tolerance anywhere."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import kfdb_reference as kr
import kfdb_scenes as ks
from kfdb_both import Both, with_scoring
from visual_sgraphs_amd import orb, synth

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
ADAPTOR = ROOT / "tests" / "_adaptor_kfdb"
SCORINGS = (kr.L1_NORM, kr.L2_NORM, kr.CHI_SQUARE, kr.BHATTACHARYYA, kr.DOT_PRODUCT)
CAPACITY, UNSUPPORTED, INVALID = -2, -3, -6
MAX_QUERY_WORDS = 12288
I32, F64, U64 = np.int32, np.float64, np.uint64
I32P, F64P, U64P = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint64)


@pytest.fixture(scope="module")
def blob_1k():
    return synth.synthetic_vocabulary(10, 3, seed=3)  # 1000 words


@pytest.fixture(scope="module")
def vocs(blob_1k):
    """scoring -> the 1000-word vocabulary with that scoring type"""
    v = {s: orb.ORBVocabulary(with_scoring(blob_1k, s)) for s in SCORINGS}
    yield v
    for x in v.values():
        x.close()


@pytest.fixture(scope="module")
def voc_big():
    """k = 11, L = 4: 14641 words, the smallest shape the loader takes (k <= 20, L <= 10) with more than 12289"""
    v = orb.ORBVocabulary(synth.synthetic_vocabulary(11, 4, seed=5))
    assert v.nwords == 14641
    yield v
    v.close()


def bits(a):
    return np.ascontiguousarray(a, F64).view(U64)


def bow(ids, vals):
    return np.array(ids, I32), np.array(vals, F64)


# ---- the scenes

@pytest.mark.parametrize("name,scoring", [(s["name"], sc) for s in ks.SCENES for sc in ks.scorings_of(s)])
def test_scene(vocs, name, scoring):
    s = ks.BY_NAME[name]
    db = Both(vocs[scoring])
    assert ks.run(s, db) == s["expect"], s["mistake"]
    db.check_state(name)
    assert db.n_states > 0
    db.close()


# ---- BowVector lengths around the 64-entry chunk

LENGTHS = (0, 1, 63, 64, 65, 128, 129, 193)
BASE = dict(zip(LENGTHS, np.cumsum((0,) + LENGTHS[:-1])))  # keyframe of length n holds words BASE[n] .. BASE[n] + n - 1
OTHER = list(range(700, 760))  # words no keyframe holds


def length_vector(n, scoring):
    """n words from BASE[n] with values k / 256; ChiSquare: every third value is 0 (its query has the same zeros, so
    vi + wi == 0 on lanes whose neighbours do have terms)"""
    ids = np.arange(BASE[n], BASE[n] + n, dtype=I32)
    vals = ((np.arange(n) * 37) % 61 + 1) / 256.0
    if scoring == kr.CHI_SQUARE:
        vals[1::3] = 0.0
    return ids, vals


def length_queries(n, scoring):
    """placement -> query: `all` the vector itself (every lane of every chunk holds a term), `last` shares only the
    last partial chunk, `none` shares nothing"""
    ids, vals = length_vector(n, scoring)
    first_of_last = 64 * ((n - 1) // 64) if n else 0
    other = np.array(OTHER[:7], I32)
    last = np.concatenate([ids[first_of_last:], other]).astype(I32)
    last_vals = np.concatenate([vals[first_of_last:][::-1], np.full(7, 0.125)])
    return {"all": (ids, vals), "last": (last, last_vals), "none": (other, np.full(7, 0.125))}


@pytest.mark.parametrize("scoring", SCORINGS)
def test_bowvector_lengths_through_the_database(vocs, scoring):
    db = Both(vocs[scoring])
    for n in LENGTHS:
        db.add(1000 + n, length_vector(n, scoring), 0)  # n = 0: a live slot of length 0
    qid, found = 1, 0
    for n in LENGTHS:
        for place, q in length_queries(n, scoring).items():
            got = db.reloc(qid, q, 0)
            loop, _ = db.nbest(qid + 1, q, [], 0, 2)
            qid += 2
            if n and place != "none":
                assert loop == [1000 + n], (n, place)  # the N-best list has no score filter
                assert db.ref.kf(1000 + n).mnPlaceRecognitionWords == (n if place == "all" else (n - 1) % 64 + 1)
                found += 1
            else:
                assert got == [] and loop == []
    assert found == 2 * (len(LENGTHS) - 1)
    db.close()


@pytest.mark.parametrize("scoring", SCORINGS)
def test_bowvector_lengths_through_vocab_score(vocs, scoring):
    voc = vocs[scoring]
    items = [length_vector(n, scoring) for n in LENGTHS]
    nonzero = 0
    for n in LENGTHS:
        for place, q in length_queries(n, scoring).items():
            got = voc.score_many(q, items)
            want = np.array([kr.score(scoring, *q, *b) for b in items], F64)
            assert np.array_equal(bits(got), bits(want)), (n, place)
            nonzero += int((want != 0).sum())
    # ChiSquare: the one entry of length 65's last chunk is one of the zeros, so that score is a sum of no terms
    assert nonzero == 2 * (len(LENGTHS) - 1) - (scoring == kr.CHI_SQUARE)
    # an empty query against everything, an empty item list
    got = voc.score_many(bow([], []), items)
    assert np.array_equal(bits(got), bits([kr.score(scoring, [], [], *b) for b in items]))
    assert len(voc.score_many(items[3], [])) == 0


def test_l2_clamp_at_a_sum_of_exactly_one_and_just_below(vocs):
    """ScoringObject.cpp:114-117: s >= 1 gives 1, anything below goes through 1 - sqrt(1 - s).  n values of 1 / sqrt(n)
    (n a power of 4) against themselves sum to exactly 1; with the last value a little smaller the sum is just below."""
    voc = vocs[kr.L2_NORM]
    db = Both(voc)
    items = []
    for n in (1, 4, 64, 256):
        ids = np.arange(n, dtype=I32) * 3
        exact = np.full(n, 1.0 / np.sqrt(n))
        below = exact.copy()
        # the values are powers of two, so the products and the sum are exact: 1 - 2^-53 for n = 1, else 1 - 2^-20 / n
        below[-1] = np.nextafter(1.0, 0) if n == 1 else below[-1] * (1 - 2.0 ** -20)
        assert kr.score(kr.L2_NORM, ids, exact, ids, exact) == 1.0
        assert 0 < kr.score(kr.L2_NORM, ids, exact, ids, below) < 1.0
        items += [(ids, exact), (ids, below)]
    for k, b in enumerate(items):
        db.add(k + 1, b, 0)
    for k, q in enumerate(items[::2]):
        got = voc.score_many(q, items)
        want = np.array([kr.score(kr.L2_NORM, *q, *b) for b in items], F64)
        assert np.array_equal(bits(got), bits(want))
        db.reloc(100 + k, q, 0)
        db.nbest(200 + k, q, [], 0, 8)
    db.close()


# ---- the largest query

def big_query(n, nwords, seed):
    rng = np.random.default_rng(seed)
    ids = np.sort(rng.choice(nwords - 3, n - 1, replace=False)).astype(I32) if n > 1 else np.zeros(0, I32)
    ids = np.concatenate([ids, [nwords - 1]]).astype(I32)  # the last query word is the last word of the vocabulary
    v = rng.random(n) + 0.05
    return ids, v / v.sum()


def test_query_sizes_up_to_the_limit_and_the_refusal_above_it(voc_big):
    nw = voc_big.nwords
    db = Both(voc_big)
    last = nw - 1
    db.add(1, bow([last - 9, last - 5, last], [0.25, 0.25, 0.5]), 0)  # found through the query's LAST word (LDS slot n - 1)
    db.add(2, bow([0, 1, 2, 3, last], [0.125, 0.125, 0.25, 0.25, 0.25]), 0)
    db.add(3, bow(range(100, 400, 3), np.full(100, 0.01)), 0)
    db.set_covisibility({1: [2, 3]})
    items = [db.ref.kf(k).bow for k in (1, 2, 3)]
    qid = 10
    for n in (1, MAX_QUERY_WORDS - 1, MAX_QUERY_WORDS):
        q = big_query(n, nw, n)
        assert len(q[0]) == n and (np.diff(q[0]) > 0).all()
        got = voc_big.score_many(q, items)
        want = np.array([kr.score(voc_big.scoring, *q, *b) for b in items], F64)
        assert np.array_equal(bits(got), bits(want)), n
        assert want[0] > 0
        assert 1 in db.reloc(qid, q, 0) or n > 1
        assert db.nbest(qid + 1, q, [], 0, 3)[0]
        qid += 2
    # one word more: refused on the host, nothing enqueued, nothing changed
    q = big_query(MAX_QUERY_WORDS + 1, nw, 99)
    for call in (lambda: db.gpu.DetectRelocalizationCandidates(qid, q, 0),
                 lambda: db.gpu.DetectNBestCandidates(qid, q, [], 0, 3), lambda: voc_big.score_many(q, items)):
        with pytest.raises(orb.VsgError) as ei:
            call()
        assert ei.value.code == UNSUPPORTED
        db.check_state("after the refusal")
    db.reloc(qid + 2, big_query(MAX_QUERY_WORDS, nw, 7), 0)
    db.close()


# ---- the second grid-stride pass: more than 4 waves x 1024 blocks of items / candidates

def test_vocab_score_of_4097_items(vocs):
    voc = vocs[kr.L1_NORM]
    q = bow([10, 11, 12, 500], [1.0, 0.5, 0.25, 0.125])
    items = []
    for c in range(4097):
        if c % 1000 == 7:
            items.append(bow([], []))  # a few empty items
        elif c % 3 == 0:
            items.append(bow([10], [(c + 1) / 8192]))
        elif c % 3 == 1:
            items.append(bow([10, 600 + c % 300], [(c + 1) / 8192, 0.5]))
        else:
            items.append(bow([3, 10, 900], [0.5, (c + 1) / 8192, 0.25]))
    got = voc.score_many(q, items)
    want = np.array([kr.score(kr.L1_NORM, *q, *b) for b in items], F64)
    assert np.array_equal(bits(got), bits(want))
    filled = np.array([len(b[0]) > 0 for b in items])
    assert len(np.unique(want[filled])) == filled.sum() == 4097 - 5  # every expected score is its own
    assert want[4096] == 4097 / 8192  # the one item of the second pass


def test_one_query_scores_more_than_4096_candidates(vocs):
    voc = vocs[kr.DOT_PRODUCT]
    n = 4100
    rng = np.random.default_rng(11)
    vals = rng.integers(1, 1 << 20, (n, 3)) / float(1 << 22)  # distinct values, sums exact in double
    db = Both(voc)
    for k in range(n):
        db.add(k + 1, (np.array([10, 11, 12], I32), vals[k]), k % 2)
    db.set_covisibility({k: [k + 1, k - 1, k + 7] for k in range(8, n - 8, 5)})
    q = bow([10, 11, 12], [0.5, 0.25, 0.25])
    got = db.reloc(1 << 40, q, 0)
    assert len(got) > 100
    assert all(k.mnRelocWords == 3 and k.mnRelocQuery == 1 << 40 for k in db.ref.kfs.values() if 1 <= k.mnId <= n)
    loop, merge = db.nbest(5, q, [5, 6], 1, 5)
    assert len(loop) == 5 and len(merge) == 5
    assert db.n_states >= 2 * n
    db.close()


# ---- the one-thread-per-keyframe kernels: the last thread of the last block

@pytest.mark.parametrize("nidx,last_id", [(255, 2 ** 32 + 5), (256, 2 ** 63 + 1), (257, 2 ** 64 - 1), (513, 2 ** 64 - 1)])
def test_last_keyframe_of_the_last_block(vocs, nidx, last_id):
    db = Both(vocs[kr.L1_NORM])
    others = list(range(1, nidx))
    db.set_map(others, [0] * len(others))  # nidx - 1 keyframes the database knows and that share nothing
    db.add(1, bow([700, 701], [0.5, 0.5]), 0)
    db.add(nidx - 1, bow([702], [1.0]), 0)
    db.add(last_id, bow([5, 6, 7], [0.5, 0.25, 0.25]), 0)
    db.set_covisibility({last_id: [nidx - 1, 1]})
    q = bow([5, 6, 7, 8], [0.25, 0.25, 0.25, 0.25])
    hi1, hi2 = (1 << 32) | 9, (2 << 32) | 9  # query ids that differ only in the high half
    assert db.reloc(hi1, q, 0) == [last_id]
    assert db.reloc(hi2, q, 0) == [last_id]
    assert db.reloc(hi2, q, 0) == []  # the same id again: the state is not reset
    assert db.nbest(hi1, q, [], 0, 2) == ([last_id], [])
    assert db.nbest(hi2, q, [], 0, 2) == ([last_id], [])
    assert db.state(last_id) == (hi2, 6, hi2, 3)
    assert len(db.ref.kfs) == nidx
    db.close()


# ---- VSG_ERR_CAPACITY, through the C entry points

SENT = 0xDEADBEEFDEADBEEF


def p(a, t):
    return a.ctypes.data_as(t) if a is not None else None


def raw_reloc(db, qid, q, m, out, cap, n_out):
    L = orb.load_library()
    return L.vsg_kfdb_detect_relocalization_candidates(db.gpu._h, qid, p(q[0], I32P), p(q[1], F64P), len(q[0]), m,
                                                       p(out, U64P), cap, C.byref(n_out) if n_out is not None else None)


def three_candidates(voc):
    db = Both(voc)
    for k, m in ((7, 0), (3, 0), (5, 0), (9, 1)):
        db.add(k, bow([5], [0.5]), m)
    return db, bow([5], [1.0])


def test_capacity_error_of_the_relocalisation_call(vocs):
    db, q = three_candidates(vocs[kr.DOT_PRODUCT])
    out, n = np.full(4, SENT, U64), C.c_int32(-77)
    assert raw_reloc(db, 20, q, 0, out, 1, n) == CAPACITY
    assert n.value == 3 and out[0] == 7 and (out[1:] == SENT).all()
    assert db.ref.DetectRelocalizationCandidates(20, *q, 0) == [7, 3, 5]
    db.check_state("cap = 1")
    assert db.reloc(21, q, 0) == [7, 3, 5]
    n = C.c_int32(-77)
    assert raw_reloc(db, 22, q, 0, None, 0, n) == CAPACITY and n.value == 3  # cap = 0, out = NULL
    db.ref.DetectRelocalizationCandidates(22, *q, 0)
    db.check_state("cap = 0")
    out, n = np.full(4, SENT, U64), C.c_int32(-77)
    assert raw_reloc(db, 23, q, 0, out, 3, n) == 0 and n.value == 3 and [int(x) for x in out] == [7, 3, 5, SENT]
    db.ref.DetectRelocalizationCandidates(23, *q, 0)
    db.check_state("cap = 3")
    # nNumCandidates = 0 with no output arrays: the walk still runs and leaves its state
    L = orb.load_library()
    nl, nm = C.c_int32(-77), C.c_int32(-77)
    assert L.vsg_kfdb_detect_n_best_candidates(db.gpu._h, 24, p(q[0], I32P), p(q[1], F64P), 1, None, 0, 0, None, 0, 0, None,
                                               C.byref(nl), None, C.byref(nm)) == 0
    assert nl.value == 0 and nm.value == 0
    assert db.ref.DetectNBestCandidates(24, *q, [], 0, 0) == ([], [])
    db.check_state("nNumCandidates = 0")
    assert db.state(9) == (23, 1, 24, 1)
    assert db.nbest(25, q, [], 0, 2) == ([7, 3], [9])
    db.close()


# ---- refusals: every one is made by the host before anything is enqueued

class Refusals:
    def __init__(self, voc):
        self.db, self.q = three_candidates(voc)
        self.L = orb.load_library()
        self.qid = 100
        self.n = 0

    def after(self, what):
        """the state is as it was, and the next queries are right"""
        self.db.check_state(what)
        self.qid += 2
        assert self.db.reloc(self.qid, self.q, 0) == [7, 3, 5], what
        assert self.db.nbest(self.qid + 1, self.q, [7], 0, 2) == ([3, 5], [9]), what
        self.n += 1


def bad_queries(nwords):
    """what -> (ids, vals, n, code): the checks of check_query / ascending_words"""
    two = np.full(2, 0.5)
    return {
        "unsorted": (np.array([6, 5], I32), two, 2, INVALID),
        "duplicate": (np.array([5, 5], I32), two, 2, INVALID),
        "negative": (np.array([-1, 5], I32), two, 2, INVALID),
        "word id = nwords": (np.array([5, nwords], I32), two, 2, INVALID),
        "n < 0": (np.array([5, 6], I32), two, -1, INVALID),
        "ids NULL": (None, two, 2, INVALID),
        "vals NULL": (np.array([5, 6], I32), None, 2, INVALID),
    }


def test_refused_queries_leave_the_outputs_and_the_state_alone(vocs, voc_big):
    r = Refusals(vocs[kr.DOT_PRODUCT])
    db, L, q = r.db, r.L, r.q
    h = db.gpu._h
    conn, badm = np.array([7], U64), np.array([1], I32)

    def reloc(ids=q[0], vals=q[1], n=1, h=h, out=True, cap=4, n_out=True):
        o, no = np.full(4, SENT, U64), C.c_int32(-77)
        rc = L.vsg_kfdb_detect_relocalization_candidates(h, 55, p(ids, I32P), p(vals, F64P), n, 0, p(o if out else None, U64P),
                                                         cap, C.byref(no) if n_out else None)
        assert (o == SENT).all() and no.value == -77
        return rc

    def nbest(ids=q[0], vals=q[1], n=1, h=h, conn=conn, n_conn=1, bad=badm, n_bad=1, nn=2, lo=True, me=True, nl=True, nm=True):
        ol, om, cl, cm = np.full(2, SENT, U64), np.full(2, SENT, U64), C.c_int32(-77), C.c_int32(-77)
        rc = L.vsg_kfdb_detect_n_best_candidates(h, 55, p(ids, I32P), p(vals, F64P), n, p(conn, U64P), n_conn, 0,
                                                 p(bad, I32P), n_bad, nn, p(ol if lo else None, U64P),
                                                 C.byref(cl) if nl else None, p(om if me else None, U64P),
                                                 C.byref(cm) if nm else None)
        assert (ol == SENT).all() and (om == SENT).all() and cl.value == -77 and cm.value == -77
        return rc
    for what, (ids, vals, n, code) in bad_queries(1000).items():
        assert reloc(ids=ids, vals=vals, n=n) == code, what
        assert nbest(ids=ids, vals=vals, n=n) == code, what
        r.after(what)
    for kw in (dict(h=None), dict(n_out=False), dict(cap=-1), dict(out=False)):
        assert reloc(**kw) == INVALID, kw
        r.after(kw)
    for kw in (dict(h=None), dict(n_conn=-1), dict(conn=None), dict(n_bad=-1), dict(bad=None), dict(nn=-1), dict(nl=False),
               dict(nm=False), dict(lo=False), dict(me=False)):
        assert nbest(**kw) == INVALID, kw
        r.after(kw)
    assert r.n == 7 + 4 + 10
    # more than 12288 words needs a vocabulary that has them
    big = Refusals(voc_big)
    h = big.db.gpu._h
    ids, vals = big_query(MAX_QUERY_WORDS + 1, voc_big.nwords, 3)
    assert reloc(ids=ids, vals=vals, n=len(ids), h=h) == UNSUPPORTED
    assert nbest(ids=ids, vals=vals, n=len(ids), h=h) == UNSUPPORTED
    big.after("12289 words")
    big.db.close()
    db.close()


def test_refused_add_set_covisibility_and_set_map_change_nothing(vocs):
    r = Refusals(vocs[kr.DOT_PRODUCT])
    db, L = r.db, r.L
    h = db.gpu._h
    NEW = 4242  # an id the database must not learn from a refused call

    def unknown(what):
        with pytest.raises(orb.VsgError) as ei:
            db.gpu.debug_state(NEW)
        assert ei.value.code == INVALID, what
        r.after(what)
    for what, (ids, vals, n, code) in bad_queries(1000).items():
        assert L.vsg_kfdb_add(h, NEW, 0, p(ids, I32P), p(vals, F64P), n) == code, what
        unknown(what)
    assert L.vsg_kfdb_add(None, NEW, 0, p(r.q[0], I32P), p(r.q[1], F64P), 1) == INVALID
    unknown("add: db NULL")
    kf, nb = np.array([7, NEW], U64), np.array([3, 5, 9], U64)

    def cov(off, h=h, kf=kf, nb=nb, n=2):
        return L.vsg_kfdb_set_covisibility(h, p(kf, U64P), p(None if off is None else np.array(off, I32), I32P), p(nb, U64P), n)
    for what, kw in (("decreasing offsets", dict(off=[0, 2, 1])), ("negative offset", dict(off=[-1, 0, 2])),
                     ("neighbours NULL with entries", dict(off=[0, 2, 3], nb=None)), ("kf_ids NULL", dict(off=[0, 2, 3], kf=None)),
                     ("offsets NULL", dict(off=None)), ("n < 0", dict(off=[0, 2, 3], n=-1)), ("db NULL", dict(off=[0, 2, 3], h=None))):
        assert cov(**kw) == INVALID, what
        unknown("set_covisibility: " + what)
    maps = np.array([1, 1], I32)
    for what, args in (("n < 0", (h, p(kf, U64P), p(maps, I32P), -1)), ("kf_ids NULL", (h, None, p(maps, I32P), 2)),
                       ("map_ids NULL", (h, p(kf, U64P), None, 2)), ("db NULL", (None, p(kf, U64P), p(maps, I32P), 2))):
        assert L.vsg_kfdb_set_map(*args) == INVALID, what
        unknown("set_map: " + what)
    # what is not refused: no keyframes, no neighbours, erase / clearMap of nothing
    assert cov([0], n=0) == 0 and cov([0, 0, 0], nb=None) == 0 and L.vsg_kfdb_set_map(h, None, None, 0) == 0
    for k, n in ((7, []), (NEW, [])):
        db.ref.set_covisibility(k, n)
    assert L.vsg_kfdb_erase(h, 777) == 0 and L.vsg_kfdb_clear_map(h, 12) == 0
    assert L.vsg_kfdb_erase(None, 7) == INVALID and L.vsg_kfdb_clear(None) == INVALID and L.vsg_kfdb_clear_map(None, 0) == INVALID
    r.after("accepted empty calls")
    assert db.gpu.debug_state(NEW)[:2] == (0, 0)  # the accepted call made it known
    db.close()


def test_refused_vocab_score_leaves_the_output_alone(vocs, voc_big):
    voc = vocs[kr.L1_NORM]
    L = orb.load_library()
    q = bow([5, 6], [0.5, 0.5])
    ids, vals = np.array([5, 7, 6, 9], I32), np.array([0.5, 0.5, 0.25, 0.75])
    off = np.array([0, 2, 4], I32)

    def score(h=voc._h, qi=q[0], qv=q[1], n=2, off=off, ids=ids, vals=vals, m=2, out=True):
        o = np.full(3, -7.0)
        rc = L.vsg_vocab_score(h, p(qi, I32P), p(qv, F64P), n, p(off, I32P), p(ids, I32P), p(vals, F64P), m,
                               p(o if out else None, F64P))
        return rc, o
    want = [kr.score(kr.L1_NORM, *q, ids[:2], vals[:2]), kr.score(kr.L1_NORM, *q, ids[2:], vals[2:])]
    refused = [("voc NULL", dict(h=None), INVALID), ("n < 0", dict(n=-1), INVALID), ("m < 0", dict(m=-1), INVALID),
               ("query ids NULL", dict(qi=None), INVALID), ("query vals NULL", dict(qv=None), INVALID),
               ("off NULL", dict(off=None), INVALID), ("out NULL", dict(out=False), INVALID),
               ("off[0] != 0", dict(off=np.array([1, 2, 4], I32)), INVALID),
               ("decreasing off", dict(off=np.array([0, 3, 2], I32)), INVALID),
               ("unsorted item ids", dict(ids=np.array([7, 5, 6, 9], I32)), INVALID),
               ("duplicate item ids", dict(ids=np.array([5, 7, 9, 9], I32)), INVALID),
               ("item id = nwords", dict(ids=np.array([5, 7, 6, 1000], I32)), INVALID),
               ("negative item id", dict(ids=np.array([-5, 7, 6, 9], I32)), INVALID),
               ("item ids NULL with entries", dict(ids=None), INVALID), ("item vals NULL with entries", dict(vals=None), INVALID),
               ("unsorted query", dict(qi=np.array([6, 5], I32)), INVALID),
               ("query id = nwords", dict(qi=np.array([6, 1000], I32)), INVALID)]
    for what, kw, code in refused:
        rc, o = score(**kw)
        assert rc == code and (o == -7.0).all(), what
        rc, o = score()  # the next call is right
        assert rc == 0 and np.array_equal(bits(o[:2]), bits(want)) and o[2] == -7.0, what
    big_ids, big_vals = big_query(MAX_QUERY_WORDS + 1, voc_big.nwords, 3)
    rc, o = score(h=voc_big._h, qi=big_ids, qv=big_vals, n=len(big_ids))
    assert rc == UNSUPPORTED and (o == -7.0).all()
    # accepted: no items (nothing written), an empty query, empty items
    rc, o = score(m=0)
    assert rc == 0 and (o == -7.0).all()
    rc, o = score(m=0, off=None, ids=None, vals=None, out=False)
    assert rc == 0
    rc, o = score(n=0, qi=None, qv=None)
    assert rc == 0 and np.array_equal(bits(o[:2]), bits([kr.score(kr.L1_NORM, [], [], [5], [1.0])] * 2))
    rc, o = score(off=np.array([0, 0, 0], I32), ids=None, vals=None)
    assert rc == 0 and np.array_equal(bits(o[:2]), bits([kr.score(kr.L1_NORM, *q, [], [])] * 2)) and o[2] == -7.0


# ---- growth of the store: the arrays start at 1024 elements and grow by 1.5x (1024 -> 1536 -> 2304)

def test_entry_arrays_grow_twice_under_long_vectors(vocs):
    rng = np.random.default_rng(21)
    db = Both(vocs[kr.L1_NORM])
    qid, entries, sizes = 1, 0, []
    for k in range(7):  # 400 entries each: 1200 crosses 1024, 1600 crosses 1536, 2400 crosses 2304
        ids = np.sort(rng.choice(1000, 400, replace=False)).astype(I32)
        v = rng.random(400) + 0.05
        db.add(k + 1, (ids, v / v.sum()), k % 2)
        entries += 400
        sizes.append(entries)
        if k == 2:
            db.set_covisibility({1: [2, 3], 3: [1]})
        for probe in (0, k):  # the oldest vector (copied at every growth) and the newest
            got = db.reloc(qid, db.ref.kf(probe + 1).bow, probe % 2)
            assert probe + 1 in got
            db.nbest(qid + 1, db.ref.kf(probe + 1).bow, [], 0, 3)
            qid += 2
    assert [s > 1024 for s in sizes].index(True) == 2 and [s > 1536 for s in sizes].index(True) == 3 and sizes[-1] > 2304
    db.erase(1)
    assert 1 not in db.reloc(qid, db.ref.kf(1).bow, 0)
    db.close()


def test_slot_arrays_grow_twice_under_one_word_vectors(vocs):
    db = Both(vocs[kr.L1_NORM])
    q = bow([100], [1.0])
    qid = 1
    for k in range(1, 1541):  # slot k - 1; the keyframe rows grow at the same counts
        db.add(k, bow([100 + k % 50], [(k % 97 + 1) / 128]), 0)
        if k == 50:
            db.set_covisibility({50: [100, 150], 100: [50]})  # rows that every later growth has to carry over
        if k in (1023, 1024, 1025, 1536, 1537, 1540):  # before, at and after each growth
            got = db.reloc(qid, q, 0)
            assert len(got) > 0 and db.ref.kf(k - k % 50).mnRelocQuery == qid
            assert len(db.nbest(qid + 1, q, [50], 0, 4)[0]) == 4
            qid += 2
    db.erase(1500)
    assert 1500 not in db.nbest(qid, q, [], 0, 40)[0]
    db.close()


# ---- the C++ adaptor

def script_bow(b):
    ids, vals = b
    return " ".join([str(len(ids))] + ["%d %s" % (int(i), float(v).hex()) for i, v in zip(ids, vals)])


def scene_script(scene, ref, lines, want):
    """The scene's operations as script lines; `want` gets the restatement's output lines"""
    for op in scene["ops"]:
        what, a = op[0], op[1:]
        if what == "add":
            lines.append("add %d %d %s" % (a[0], a[3], script_bow((a[1], a[2]))))
            ref.add(a[0], a[1], a[2], a[3])
        elif what == "erase":
            lines.append("erase %d" % a[0])
            ref.erase(a[0])
        elif what == "cov":
            for k, nb in a[0].items():
                lines.append("cov %d %d %s" % (k, len(nb), " ".join(str(x) for x in nb)))
                ref.set_covisibility(k, nb)
        elif what == "reloc":
            lines.append("reloc %d %d %s" % (a[0], a[3], script_bow((a[1], a[2]))))
            want.append("reloc" + "".join(" %d" % x for x in ref.DetectRelocalizationCandidates(a[0], a[1], a[2], a[3])))
        elif what == "nbest":
            lines.append("nbest %d %d %d %d %s %d %s %s" % (a[0], a[4], a[5], len(a[3]), " ".join(str(x) for x in a[3]),
                                                          len(a[6]), " ".join(str(x) for x in a[6]), script_bow((a[1], a[2]))))
            loop, merge = ref.DetectNBestCandidates(a[0], a[1], a[2], a[3], a[4], a[5], a[6])
            want.append("nbest" + "".join(" %d" % x for x in loop) + " |" + "".join(" %d" % x for x in merge))
        else:
            raise ValueError(what)


def test_cpp_adaptor_equals_the_restatement(blob_1k, tmp_path):
    subprocess.check_call(["make", "-C", str(ADAPTOR)], stdout=subprocess.DEVNULL)
    scoring = kr.L1_NORM
    ref = kr.KeyFrameDatabase(scoring)
    lines, want = [], []
    # two directed scenes: ten of eleven neighbours, and ids in the high half of 64 bits
    scene_script(ks.BY_NAME["eleventh_neighbour"], ref, lines, want)
    lines.append("clear")
    ref.clear()
    scene_script(ks.BY_NAME["keyframe_id_high_half"], ref, lines, want)
    assert want[0] == "nbest 20 1 12 |" and want[1] == "reloc %d %d" % (2 ** 32 + 5, 2 ** 64 - 1)
    lines.append("clear")
    ref.clear()
    # a short stretch of a scripted database on random BowVectors
    rng = np.random.default_rng(8)

    def rand_bow(n):
        ids = np.sort(rng.choice(300, n, replace=False))
        v = rng.random(n) + 0.05
        return [int(i) for i in ids], [float(x) for x in v / v.sum()]
    bows = {k: rand_bow(40) for k in range(101, 131)}
    bows[105] = ([], [])  # an empty BowVector
    present = []
    for k in range(101, 121):
        scene_script(dict(ops=[("add", k, *bows[k], k % 2)]), ref, lines, want)
        present.append(k)
    lines.append("setmap 2 103 1 104 0")
    ref.set_map(103, 1), ref.set_map(104, 0)
    lines.append("setmap 0")
    for k in present[::2]:
        scene_script(dict(ops=[("cov", {k: [x for x in (k + 1, k - 1, k + 2, 9000 + k) if x != 105]})]), ref, lines, want)
    scene_script(dict(ops=[("cov", {102: []})]), ref, lines, want)  # an empty neighbour list
    qid = 500
    for step in range(40):
        k = int(rng.integers(101, 131))
        ops = []
        if step % 8 == 3 and k in present:
            ops.append(("erase", k))
            present.remove(k)
        elif step % 8 == 6 and k not in present:
            ops.append(("add", k, *bows[k], k % 2))
            present.append(k)
        elif step % 2:
            ops.append(("reloc", qid, *bows[k], step % 2))
        else:
            conn = [] if step % 4 == 0 else [k + 1, k - 1]  # an empty `connected` every other time
            bad = [] if step % 3 else [1]  # and an empty `bad_maps`
            ops.append(("nbest", k, *bows[k], conn, k % 2, 0 if step == 20 else 3, bad))  # once nNumCandidates = 0
        qid += 1
        scene_script(dict(ops=ops), ref, lines, want)
    lines.append("clearmap 1")
    ref.clearMap(1)
    scene_script(dict(ops=[("reloc", 900, *bows[102], 0), ("nbest", 901, *bows[102], [], 0, 4, []),
                           ("reloc", 902, [], [], 0)]), ref, lines, want)
    for a, b in ((bows[101], bows[102]), (bows[101], bows[101]), (bows[105], bows[101]), (bows[101], bows[105])):
        lines.append("score %s %s" % (script_bow(a), script_bow(b)))
        want.append("score " + float(kr.score(scoring, *a, *b)).hex())
    assert sum(1 for w in want if w not in ("reloc", "nbest |")) > 30  # most queries find something
    vf, sf, of = tmp_path / "voc.bin", tmp_path / "script.txt", tmp_path / "out.txt"
    vf.write_bytes(with_scoring(blob_1k, scoring))
    sf.write_text("\n".join(lines) + "\n")
    r = subprocess.run([str(ADAPTOR / "kfdb_check"), str(vf), str(sf), str(of)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
    got = of.read_text().splitlines()
    assert len(got) == len(want)
    for g, w in zip(got, want):
        if w.startswith("score"):
            assert float.fromhex(g.split()[1]).hex() == float.fromhex(w.split()[1]).hex(), (g, w)
        else:
            assert g == w
