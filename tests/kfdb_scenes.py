"""Hand-built scenes for the KeyFrameDatabase, as plain data: operations, queries and the expected results.

Every scene exists to catch ONE named mistake.  tests/test_kfdb_scenes.py shows on the CPU that the restatement
(tests/kfdb_reference.py) gives the expected results and that the restatement WITH that mistake (MISTAKES below) does
not; tests/test_gpu_kfdb_edges.py then runs the same scenes on the device database.

Scores are chosen, not hoped for: with one shared word w and a query ([w], [1.0]), a keyframe ([w], [x]) with
0 <= x <= 1 scores exactly x under DotProduct AND under L1 (-(|1 - x| - 1 - x) / 2 = x).  All values are binary
fractions, exact in float32.  A scene with scoring None holds under both; the others name their scoring.

Operations (tuples):
  ("add", kf, ids, vals, map)            ("erase", kf)          ("clear",)          ("clear_map", map)
  ("set_map", [kf...], [map...])         ("cov", {kf: [neighbours...]})
  ("reloc", query_id, ids, vals, map)                               -> list of ids
  ("nbest", query_id, ids, vals, connected, map, n, bad_maps)       -> (loop ids, merge ids)
  ("state", kf)   -> (mnRelocQuery, mnRelocWords, mnPlaceRecognitionQuery, mnPlaceRecognitionWords)
`expect` lists the results of the reloc / nbest / state operations in order."""
import numpy as np

import kfdb_reference as kr

F32 = np.float32
NEXT_075 = float(np.nextafter(F32(0.75), F32(1)))  # the float32 after 0.75
EPS24 = 2.0 ** -24
BIG = 2 ** 32


def one(w, x=1.0):
    return [w], [float(x)]


def uni(words, x=0.5):
    words = list(words)
    return words, [float(x)] * len(words)


def first(words, x):
    """words with value x on the first and 0 on the rest: a DotProduct with a like query sees only the first"""
    words = list(words)
    return words, [float(x)] + [0.0] * (len(words) - 1)


SCENES = [
    dict(name="filter_075", scoring=None, mistake=">= instead of > at the 0.75 * bestAccScore filter",
         ops=[("add", 1, *one(5, 1.0), 0), ("add", 2, *one(5, 0.75), 0), ("add", 3, *one(5, NEXT_075), 0),
              ("reloc", 10, *one(5), 0)],
         expect=[[1, 3]]),
    dict(name="gate_08", scoring=kr.DOT_PRODUCT, mistake=">= instead of > at the minCommonWords gate",
         # maxCommonWords 10 -> minCommonWords 8: 8 words are out, 9 are in
         ops=[("add", 1, *first(range(10), 1.0), 0), ("add", 2, *first(range(8), 0.875), 0),
              ("add", 3, *first(range(9), 0.875), 0),
              ("reloc", 10, *first(range(10), 1.0), 0), ("nbest", 11, *first(range(10), 1.0), [], 0, 3, [])],
         expect=[[1, 3], ([1, 3], [])]),
    dict(name="best_tie_own", scoring=None, mistake=">= instead of > when a neighbour ties the best score",
         ops=[("add", 1, *one(5, 0.5), 0), ("add", 2, *one(5, 0.5), 0), ("add", 3, *one(5, 0.5), 0),
              ("cov", {1: [2, 3]}), ("reloc", 10, *one(5), 0), ("nbest", 11, *one(5), [], 0, 1, [])],
         expect=[[1], ([1], [])]),
    dict(name="best_tie_neighbours", scoring=None, mistake=">= instead of > when a neighbour ties the best score",
         # 900 is a neighbour the database never saw otherwise: it takes no part
         ops=[("add", 1, *one(5, 0.25), 0), ("add", 2, *one(5, 0.5), 0), ("add", 3, *one(5, 0.5), 0),
              ("cov", {1: [900, 2, 3]}), ("reloc", 10, *one(5), 0), ("nbest", 11, *one(5), [], 0, 1, [])],
         expect=[[2], ([2], [])]),
    dict(name="acc_order", scoring=None, mistake="neighbours summed before the own score",
         # float32: 1 + 2^-24 + 2^-24 = 1 in this order, 1.0000001 when the neighbours are added to each other first
         ops=[("add", 4, *one(5, 1.0), 0), ("add", 1, *one(5, 1.0), 0), ("add", 2, *one(5, EPS24), 0),
              ("add", 3, *one(5, EPS24), 0), ("cov", {1: [2, 3]}), ("nbest", 10, *one(5), [], 0, 4, [])],
         expect=[([4, 1, 2, 3], [])]),
    dict(name="stable_sort", scoring=None, mistake="ties of accScore ordered by id, not by list order",
         ops=[("add", 7, *one(5, 0.5), 0), ("add", 3, *one(5, 0.5), 0), ("add", 5, *one(5, 0.5), 1),
              ("nbest", 10, *one(5), [], 0, 3, []), ("nbest", 11, *one(5), [], 1, 3, [0]),
              ("reloc", 12, *one(5), 0)],
         expect=[([7, 3], [5]), ([5], []), [7, 3]]),
    dict(name="eleventh_neighbour", scoring=None, mistake="11th neighbour used",
         # 1 scores 0.5 + 10/64 = 0.65625 < 0.6875 of keyframe 20; with the 11th neighbour (0.375) it would lead.
         # 998 and 999 are neighbours the database never saw otherwise.
         ops=[("add", 1, *one(5, 0.5), 0)] + [("add", k, *one(5, 1 / 64), 0) for k in range(2, 12)] +
             [("add", 12, *one(5, 0.375), 0), ("add", 20, *one(5, 0.6875), 0),
              ("cov", {1: list(range(2, 13)), 20: [999, 998]}), ("nbest", 10, *one(5), [], 0, 3, [])],
         expect=[([20, 1, 12], [])]),
    dict(name="double_add_erase", scoring=None, mistake="erase takes the newest slot",
         # word 3 lists [1, 2, 1]; erase(1) removes the FIRST entry of 1 and leaves [2, 1].  Word 4 is gone; word 9
         # (only in the first vector) stays findable: the walk counts it (the state), the score against the last
         # vector is 0 and 0 > 0.75 * 0 fails.
         ops=[("add", 1, *uni([3, 9], 1.0), 0), ("add", 2, *one(3, 1.0), 0), ("add", 1, *uni([3, 4], 1.0), 0),
              ("erase", 1), ("reloc", 10, *one(3), 0), ("reloc", 11, *one(4), 0), ("reloc", 12, *one(9), 0),
              ("state", 1)],
         expect=[[2, 1], [], [], (12, 1, 0, 0)]),
    dict(name="tombstone_not_counted", scoring=kr.DOT_PRODUCT, mistake="tombstoned entry still counted",
         # after the erase keyframe 1 holds 11 12 13 20 (first vector, 10 tombstoned) and 10 (second vector, 30
         # tombstoned): 4 of the query's words against keyframe 2's 5 -> not above minCommonWords = 4
         ops=[("add", 1, *first([10, 11, 12, 13, 20], 1.0), 0), ("add", 1, *first([10, 30], 1.0), 0),
              ("add", 2, *first([10, 11, 12, 13, 14], 1.0), 0), ("erase", 1),
              ("reloc", 10, *first([10, 11, 12, 13, 14], 1.0), 0), ("state", 1), ("reloc", 11, *one(30), 0)],
         expect=[[2], (10, 4, 0, 0), []]),
    dict(name="dead_bow_slot", scoring=None, mistake="score read from the oldest slot",
         # the last vector's slot dies in the erase, the first one lives: found through word 5, scored 1.0 on word 6
         ops=[("add", 1, *one(5, 0.25), 0), ("add", 1, *one(6, 1.0), 0), ("add", 2, *one(5, 0.5), 0), ("erase", 1),
              ("reloc", 10, *uni([5, 6], 1.0), 0), ("nbest", 11, *uni([5, 6], 1.0), [], 0, 1, [])],
         expect=[[1], ([1], [])]),
    dict(name="tombstones_one_by_one", scoring=None, mistake="erase drops every entry of the keyframe",
         # every score is 0.5: keyframe 2 has 0.25 on both words, keyframe 1's last vector 0.5 on its one word
         ops=[("add", 2, *uni([1, 2], 0.25), 0), ("add", 1, *uni([1, 2]), 0), ("add", 1, *uni([1]), 0), ("erase", 1),
              ("reloc", 10, *uni([1, 2], 1.0), 0), ("state", 1), ("add", 1, *uni([2]), 0), ("erase", 1),
              ("reloc", 11, *uni([1, 2], 1.0), 0), ("state", 1), ("erase", 1), ("reloc", 12, *uni([1, 2], 1.0), 0),
              ("state", 1), ("erase", 1), ("reloc", 13, *uni([1, 2], 1.0), 0)],
         expect=[[2, 1], (10, 2, 0, 0), [2, 1], (11, 2, 0, 0), [2], (12, 1, 0, 0), [2]]),
    dict(name="clear_drops_postings", scoring=None, mistake="clear leaves the postings",
         # after clear() the store restarts: keyframe 3's new vector takes slot 0, under the stale rows of 1 and 2
         ops=[("add", 1, *one(5, 0.5), 0), ("add", 2, *one(5, 1.0), 0), ("add", 3, *one(7, 1.0), 0),
              ("reloc", 10, *one(5), 0), ("clear",), ("reloc", 11, *one(5), 0), ("add", 3, *one(5, 0.25), 0),
              ("reloc", 12, *one(5), 0), ("nbest", 13, *one(5), [], 0, 3, []), ("state", 1), ("state", 2)],
         expect=[[2], [], [3], ([3], []), (10, 1, 0, 0), (10, 1, 0, 0)]),
    dict(name="clear_keeps_state", scoring=None, mistake="clear resets the query state",
         ops=[("add", 1, *one(5), 0), ("reloc", 7, *one(5), 0), ("clear",), ("add", 1, *one(5), 0),
              ("reloc", 7, *one(5), 0), ("state", 1)],
         expect=[[1], [], (7, 2, 0, 0)]),
    dict(name="set_map", scoring=None, mistake="set_map ignored",
         # set_map before the first add, erase of an id never seen, clearMap of a map without keyframes, erase twice
         ops=[("set_map", [1], [5]), ("add", 1, *one(5), 0), ("erase", 77), ("clear_map", 9),
              ("reloc", 10, *one(5), 0), ("set_map", [1], [2]), ("reloc", 11, *one(5), 0), ("reloc", 12, *one(5), 2),
              ("nbest", 13, *one(5), [], 0, 2, []), ("nbest", 14, *one(5), [], 0, 2, [2]), ("erase", 1), ("erase", 1),
              ("reloc", 15, *one(5), 2)],
         expect=[[1], [], [1], ([], [1]), ([], []), []]),
    dict(name="erase_twice", scoring=None, mistake="a second erase without an add between does nothing",
         ops=[("add", 1, *one(5), 0), ("add", 2, *one(5), 0), ("add", 1, *one(5), 0), ("reloc", 10, *one(5), 0),
              ("erase", 1), ("reloc", 11, *one(5), 0), ("erase", 1), ("reloc", 12, *one(5), 0), ("erase", 1),
              ("reloc", 13, *one(5), 0)],
         expect=[[1], [2, 1], [2], [2]]),
    dict(name="query_id_high_half", scoring=None, mistake="query id compared in 32 bits",
         ops=[("add", 1, *one(5), 0), ("reloc", BIG + 7, *one(5), 0), ("reloc", 7, *one(5), 0),
              ("reloc", 2 * BIG + 7, *one(5), 0), ("nbest", 2 ** 63 + 9, *one(5), [], 0, 1, []),
              ("nbest", 9, *one(5), [], 0, 1, []), ("state", 1)],
         expect=[[1], [1], [1], ([1], []), ([1], []), (2 * BIG + 7, 1, 9, 1)]),
    dict(name="keyframe_id_high_half", scoring=None, mistake="keyframe id truncated to 32 bits",
         ops=[("add", BIG + 5, *one(5, 1.0), 0), ("add", 5, *one(5, 0.25), 0), ("add", 2 ** 63 + 1, *one(5, 1.0), 1),
              ("add", 2 ** 64 - 1, *one(5, 0.75), 0), ("cov", {5: [2 ** 64 - 1]}),
              ("reloc", 10, *one(5), 0), ("nbest", 11, *one(5), [BIG + 5], 0, 3, [])],
         # reloc: 5 accumulates 1.0 and hands over to 2^64 - 1, whose own 0.75 is not above 0.75; 2^63 + 1 is in the other map
         expect=[[BIG + 5, 2 ** 64 - 1], ([2 ** 64 - 1], [2 ** 63 + 1])]),
    dict(name="connected_keyframe", scoring=None, mistake="connected keyframe walked like any other",
         ops=[("add", 1, *uni([1, 2, 3]), 0), ("add", 2, *uni([1, 2, 3]), 0),
              ("nbest", 50, *uni([1, 2, 3], 1.0), [1, 777], 0, 3, []), ("state", 1), ("state", 2)],
         expect=[([2], []), (0, 0, 0, 1), (0, 0, 50, 3)]),
    dict(name="connected_max_words", scoring=None, mistake="maxCommonWords taken over connected keyframes too",
         # the connected keyframe shares 10 words, the other one 5: maxCommonWords is 5, not 10 (minCommonWords 8)
         ops=[("add", 1, *uni(range(10), 0.125), 0), ("add", 2, *uni(range(5), 0.125), 0),
              ("nbest", 50, *uni(range(10), 0.125), [1], 0, 3, []), ("state", 1), ("state", 2)],
         expect=[([2], []), (0, 0, 0, 1), (0, 0, 50, 5)]),
    dict(name="repeated_query_id", scoring=None, mistake="words restart at every query",
         ops=[("add", 1, *uni([1, 2]), 0), ("reloc", 9, *uni([1, 2], 1.0), 0), ("reloc", 9, *uni([1, 2], 1.0), 0),
              ("state", 1), ("nbest", 9, *uni([1, 2], 1.0), [], 0, 1, []), ("nbest", 9, *uni([1, 2], 1.0), [], 0, 1, []),
              ("state", 1)],
         expect=[[1], [], (9, 4, 0, 0), ([1], []), ([], []), (9, 4, 9, 4)]),
    dict(name="chi_square_zero_terms", scoring=kr.CHI_SQUARE, mistake="ChiSquare adds the 0 / 0 term",
         # words 1 and 3: vi + wi == 0, the term is skipped; the score is 2 * (0.5 * 0.5 / 1) = 0.5
         ops=[("add", 1, [1, 2, 3], [0.0, 0.5, 0.0], 0), ("reloc", 10, [1, 2, 3], [0.0, 0.5, 0.0], 0),
              ("nbest", 11, [1, 2, 3], [0.0, 0.5, 0.0], [], 0, 1, [])],
         expect=[[1], ([1], [])]),
]

BY_NAME = {s["name"]: s for s in SCENES}


def scorings_of(scene):
    return (kr.L1_NORM, kr.DOT_PRODUCT) if scene["scoring"] is None else (scene["scoring"],)


class RefDriver:
    """The restatement (or a mistaken variant of it) behind the interface run() drives."""

    def __init__(self, db):
        self.ref = db

    def add(self, kf, bow, m):
        self.ref.add(kf, *bow, m)

    def erase(self, kf):
        self.ref.erase(kf)

    def clear(self):
        self.ref.clear()

    def clear_map(self, m):
        self.ref.clearMap(m)

    def set_map(self, kfs, maps):
        for k, m in zip(kfs, maps):
            self.ref.set_map(k, m)

    def set_covisibility(self, neigh):
        for k, n in neigh.items():
            self.ref.set_covisibility(k, n)

    def state(self, kf):
        k = self.ref.kf(kf)
        return k.mnRelocQuery, k.mnRelocWords, k.mnPlaceRecognitionQuery, k.mnPlaceRecognitionWords

    def reloc(self, qid, bow, m):
        return self.ref.DetectRelocalizationCandidates(qid, *bow, m)

    def nbest(self, qid, bow, conn, m, n, bad=()):
        return self.ref.DetectNBestCandidates(qid, *bow, conn, m, n, bad)


def bow(ids, vals):
    return np.array(ids, np.int32), np.array(vals, np.float64)


def run(scene, db):
    """Drive `db` (a RefDriver, or the Both of tests/kfdb_both.py) through the scene; the results of its queries and
    state reads, in order."""
    out = []
    for op in scene["ops"]:
        what, a = op[0], op[1:]
        if what == "add":
            db.add(a[0], bow(a[1], a[2]), a[3])
        elif what == "erase":
            db.erase(a[0])
        elif what == "clear":
            db.clear()
        elif what == "clear_map":
            db.clear_map(a[0])
        elif what == "set_map":
            db.set_map(a[0], a[1])
        elif what == "cov":
            db.set_covisibility(a[0])
        elif what == "reloc":
            out.append(db.reloc(a[0], bow(a[1], a[2]), a[3]))
        elif what == "nbest":
            loop, merge = db.nbest(a[0], bow(a[1], a[2]), a[3], a[4], a[5], a[6])
            out.append((loop, merge))
        elif what == "state":
            out.append(db.state(a[0]))
        else:
            raise ValueError(what)
    return out


# ---- the restatement with one mistake each

class FilterGe(kr.KeyFrameDatabase):
    def _retained(self, accScore, minScoreToRetain):
        return accScore >= minScoreToRetain


class GateGe(kr.KeyFrameDatabase):
    def _passes_gate(self, words, minCommonWords):
        return words >= minCommonWords


class BestGe(kr.KeyFrameDatabase):
    def _better(self, score, bestScore):
        return score >= bestScore


class NeighboursFirst(kr.KeyFrameDatabase):
    def _acc_chain(self, si, neighbour_scores):
        acc = F32(0)
        for sc in neighbour_scores:
            acc = F32(acc + sc)
        return F32(acc + si)


class SortById(kr.KeyFrameDatabase):
    def _sorted(self, acc_list):
        return sorted(acc_list, key=lambda p: (-float(p[0]), p[1].mnId))


class ElevenNeighbours(kr.KeyFrameDatabase):
    N_COVIS = 11


class EraseNewest(kr.KeyFrameDatabase):
    def _erase_pos(self, lst, k):
        hits = [p for p, x in enumerate(lst) if x is k]
        return hits[-1] if hits else None


class TombstonesIgnored(kr.KeyFrameDatabase):
    """A slot counts with all its entries until every one of them is gone.  The scene's only erase leaves both slots of
    the keyframe partly alive, so with this mistake that erase removes nothing."""

    def erase(self, kf_id):
        k = self.kf(kf_id)
        held = {w for w, lst in self.inv.items() if any(x is k for x in lst)}
        if held - set(int(w) for w in k.bow[0]):
            return
        super().erase(kf_id)


class OldestSlotScore(kr.KeyFrameDatabase):
    """The score uses the vector of the keyframe's oldest live slot instead of its last BowVector."""

    def add(self, kf_id, ids, vals, map_id):
        k = self.kf(kf_id)
        had = any(x is k for lst in self.inv.values() for x in lst)
        super().add(kf_id, ids, vals, map_id)
        if not had:
            k.oldest = k.bow

    def _score(self, q_ids, q_vals, k):
        return kr.score(self.scoring, q_ids, q_vals, *k.oldest)


class EraseAll(kr.KeyFrameDatabase):
    def erase(self, kf_id):
        k = self.kf(kf_id)
        for w in self.inv:
            self.inv[w] = [x for x in self.inv[w] if x is not k]


class ClearKeepsPostings(kr.KeyFrameDatabase):
    def clear(self):
        pass


class ClearResetsState(kr.KeyFrameDatabase):
    def clear(self):
        super().clear()
        for k in self.kfs.values():
            k.mnRelocQuery = k.mnRelocWords = k.mnPlaceRecognitionQuery = k.mnPlaceRecognitionWords = 0


class SetMapIgnored(kr.KeyFrameDatabase):
    def set_map(self, kf_id, map_id):
        self.kf(kf_id)


class EraseOnce(kr.KeyFrameDatabase):
    def __init__(self, scoring):
        super().__init__(scoring)
        self.erased = set()

    def add(self, kf_id, ids, vals, map_id):
        self.erased.discard(kf_id)
        super().add(kf_id, ids, vals, map_id)

    def erase(self, kf_id):
        if kf_id not in self.erased:
            self.erased.add(kf_id)
            super().erase(kf_id)


class Query32(kr.KeyFrameDatabase):
    def _same_query(self, stored, query_id):
        return (stored ^ query_id) & 0xFFFFFFFF == 0


class KeyFrameId32(kr.KeyFrameDatabase):
    def kf(self, kf_id):
        return super().kf(kf_id & 0xFFFFFFFF)

    def _is_connected(self, k, connected):
        return k.mnId in {c & 0xFFFFFFFF for c in connected}


class ConnectedWalked(kr.KeyFrameDatabase):
    def _is_connected(self, k, connected):
        return False


class ConnectedInMax(kr.KeyFrameDatabase):
    """maxCommonWords also sees the words a connected keyframe shares with the query."""

    def DetectNBestCandidates(self, query_kf_id, q_ids, q_vals, connected_ids, map_id, nNumCandidates, bad_map_ids=()):
        shared = {}
        for w in q_ids:
            for k in self.inv.get(int(w), []):
                if k.mnId in set(connected_ids):
                    shared[k.mnId] = shared.get(k.mnId, 0) + 1
        self.floor = int(F32(max(shared.values(), default=0)) * F32(0.8))
        return super().DetectNBestCandidates(query_kf_id, q_ids, q_vals, connected_ids, map_id, nNumCandidates, bad_map_ids)

    def _passes_gate(self, words, minCommonWords):
        return words > max(minCommonWords, self.floor)


class WordsRestart(kr.KeyFrameDatabase):
    def _same_query(self, stored, query_id):
        return False


class ChiSquareZeroTerm(kr.KeyFrameDatabase):
    def _score(self, q_ids, q_vals, k):
        s = 0.0
        other = dict(zip((int(w) for w in k.bow[0]), k.bow[1]))
        for w, vi in zip(q_ids, q_vals):
            if int(w) in other:
                wi = other[int(w)]
                s += vi * wi / (vi + wi) if vi + wi != 0.0 else float("nan")
        return 2. * s


MISTAKES = {
    "filter_075": FilterGe, "gate_08": GateGe, "best_tie_own": BestGe, "best_tie_neighbours": BestGe,
    "acc_order": NeighboursFirst, "stable_sort": SortById, "eleventh_neighbour": ElevenNeighbours,
    "double_add_erase": EraseNewest, "tombstone_not_counted": TombstonesIgnored, "dead_bow_slot": OldestSlotScore,
    "tombstones_one_by_one": EraseAll, "clear_drops_postings": ClearKeepsPostings,
    "clear_keeps_state": ClearResetsState, "set_map": SetMapIgnored, "erase_twice": EraseOnce,
    "query_id_high_half": Query32, "keyframe_id_high_half": KeyFrameId32, "connected_keyframe": ConnectedWalked,
    "connected_max_words": ConnectedInMax,
    "repeated_query_id": WordsRestart, "chi_square_zero_terms": ChiSquareZeroTerm,
}
