"""Python restatement of DBoW2's scoring (ScoringObject.cpp) and of the reference's KeyFrameDatabase
(orb_slam3/src/KeyFrameDatabase.cc:36-96, 592-830), with the per-keyframe query state the queries read and write.

Python floats are IEEE doubles; the reference's float steps (si, accScore, 0.75f * bestAccScore, maxCommonWords * 0.8f)
use np.float32.  The model is written as the reference is: std::list posting lists walked word by word."""
import math
import sys

import numpy as np

L1_NORM, L2_NORM, CHI_SQUARE, KL, BHATTACHARYYA, DOT_PRODUCT = range(6)
LOG_EPS = math.log(sys.float_info.epsilon)  # GeneralScoring::LOG_EPS = log(DBL_EPSILON)
F32 = np.float32


def _pairs(ids, vals):
    return [(int(i), float(v)) for i, v in zip(ids, vals)]


def score(scoring, a_ids, a_vals, b_ids, b_vals):
    """ScoringObject.cpp score(v1 = a, v2 = b): the merge loop in ascending word id, one chain of double additions."""
    v1, v2 = _pairs(a_ids, a_vals), _pairs(b_ids, b_vals)
    i = j = 0
    s = 0.0
    if scoring == KL:
        while i < len(v1) and j < len(v2):
            (a, vi), (b, wi) = v1[i], v2[j]
            if a == b:
                if vi != 0 and wi != 0:
                    s += vi * math.log(vi / wi)
                i += 1
                j += 1
            elif a < b:
                s += vi * (math.log(vi) - LOG_EPS)
                i += 1
            else:
                while j < len(v2) and v2[j][0] < a:
                    j += 1
        for a, vi in v1[i:]:
            if vi != 0:
                s += vi * (math.log(vi) - LOG_EPS)
        return s
    while i < len(v1) and j < len(v2):
        (a, vi), (b, wi) = v1[i], v2[j]
        if a == b:
            if scoring == L1_NORM:
                s += abs(vi - wi) - abs(vi) - abs(wi)
            elif scoring in (L2_NORM, DOT_PRODUCT):
                s += vi * wi
            elif scoring == CHI_SQUARE:
                if vi + wi != 0.0:
                    s += vi * wi / (vi + wi)
            elif scoring == BHATTACHARYYA:
                s += math.sqrt(vi * wi)
            i += 1
            j += 1
        elif a < b:
            while i < len(v1) and v1[i][0] < b:  # v1.lower_bound(v2_it->first)
                i += 1
        else:
            while j < len(v2) and v2[j][0] < a:
                j += 1
    if scoring == L1_NORM:
        return -s / 2.0
    if scoring == L2_NORM:
        return 1.0 if s >= 1 else 1.0 - math.sqrt(1.0 - s)
    if scoring == CHI_SQUARE:
        return 2. * s
    return s


class KeyFrame:
    """The KeyFrame members the database reads and writes (KeyFrame.cc:33,46: all query state starts at 0;
    mRelocScore, never initialised in the reference, is defined as 0)."""

    def __init__(self, kf_id):
        self.mnId = kf_id
        self.map = -1
        self.bow = ([], [])
        self.covis = []  # GetBestCovisibilityKeyFrames(10)
        self.mnRelocQuery = 0
        self.mnRelocWords = 0
        self.mRelocScore = F32(0)
        self.mnPlaceRecognitionQuery = 0
        self.mnPlaceRecognitionWords = 0
        self.mPlaceRecognitionScore = F32(0)


class KeyFrameDatabase:
    def __init__(self, scoring):
        self.scoring = scoring
        self.inv = {}  # word -> list of KeyFrame (mvInvertedFile)
        self.kfs = {}  # every keyframe id seen -> KeyFrame (the objects outlive their database entries)

    # ---- seams: every default is the reference's own behaviour.  tests/kfdb_scenes.py overrides one at a time, to show
    # that a directed scene tells the reference from one named mistake.
    N_COVIS = 10  # GetBestCovisibilityKeyFrames(10)

    def _same_query(self, stored, query_id):
        return stored == query_id

    def _passes_gate(self, words, minCommonWords):
        return words > minCommonWords

    def _retained(self, accScore, minScoreToRetain):
        return accScore > minScoreToRetain

    def _better(self, score, bestScore):
        return score > bestScore

    def _acc_chain(self, si, neighbour_scores):
        accScore = si
        for sc in neighbour_scores:
            accScore = F32(accScore + sc)
        return accScore

    def _sorted(self, acc_list):
        return sorted(acc_list, key=lambda p: float(p[0]), reverse=True)  # stable, like std::list::sort(compFirst)

    def _erase_pos(self, lst, k):
        for p, x in enumerate(lst):
            if x is k:
                return p
        return None

    def _is_connected(self, k, connected):
        return k.mnId in connected

    def kf(self, kf_id):
        k = self.kfs.get(kf_id)
        if k is None:
            k = self.kfs[kf_id] = KeyFrame(kf_id)
        return k

    # ---- :36-96
    def add(self, kf_id, ids, vals, map_id):
        k = self.kf(kf_id)
        k.map = map_id
        k.bow = (list(ids), list(vals))
        for w in k.bow[0]:
            self.inv.setdefault(int(w), []).append(k)

    def erase(self, kf_id):
        k = self.kf(kf_id)
        for w in k.bow[0]:
            lst = self.inv.get(int(w), [])
            p = self._erase_pos(lst, k)
            if p is not None:
                del lst[p]

    def clear(self):
        self.inv = {}

    def clearMap(self, map_id):
        for w in self.inv:
            self.inv[w] = [x for x in self.inv[w] if x.map != map_id]

    def set_map(self, kf_id, map_id):
        self.kf(kf_id).map = map_id

    def set_covisibility(self, kf_id, neighbours):
        self.kf(kf_id).covis = [self.kf(n) for n in list(neighbours)[:self.N_COVIS]]

    def _score(self, q_ids, q_vals, k):
        return score(self.scoring, q_ids, q_vals, k.bow[0], k.bow[1])

    # ---- :719-830
    def DetectRelocalizationCandidates(self, query_id, q_ids, q_vals, map_id):
        sharing = []
        for w in q_ids:
            for k in self.inv.get(int(w), []):
                if not self._same_query(k.mnRelocQuery, query_id):
                    k.mnRelocWords = 0
                    k.mnRelocQuery = query_id
                    sharing.append(k)
                k.mnRelocWords += 1
        if not sharing:
            return []
        maxCommonWords = max(0, max(k.mnRelocWords for k in sharing))
        minCommonWords = int(F32(maxCommonWords) * F32(0.8))
        scored = []
        for k in sharing:
            if self._passes_gate(k.mnRelocWords, minCommonWords):
                si = F32(self._score(q_ids, q_vals, k))
                k.mRelocScore = si
                scored.append((si, k))
        if not scored:
            return []
        acc_list = []
        bestAccScore = F32(0)
        for si, k in scored:
            bestScore = si
            best = k
            seen = [k2 for k2 in k.covis if self._same_query(k2.mnRelocQuery, query_id)]
            accScore = self._acc_chain(si, [k2.mRelocScore for k2 in seen])
            for k2 in seen:
                if self._better(k2.mRelocScore, bestScore):
                    best = k2
                    bestScore = k2.mRelocScore
            acc_list.append((accScore, best))
            if accScore > bestAccScore:
                bestAccScore = accScore
        minScoreToRetain = F32(F32(0.75) * bestAccScore)
        added, out = set(), []
        for s, k in acc_list:
            if self._retained(s, minScoreToRetain):
                if k.map != map_id:
                    continue
                if k.mnId not in added:
                    out.append(k.mnId)
                    added.add(k.mnId)
        return out

    # ---- :592-717
    def DetectNBestCandidates(self, query_kf_id, q_ids, q_vals, connected_ids, map_id, nNumCandidates,
                              bad_map_ids=()):
        connected = set(connected_ids)
        sharing = []
        for w in q_ids:
            for k in self.inv.get(int(w), []):
                if not self._same_query(k.mnPlaceRecognitionQuery, query_kf_id):
                    k.mnPlaceRecognitionWords = 0
                    if not self._is_connected(k, connected):
                        k.mnPlaceRecognitionQuery = query_kf_id
                        sharing.append(k)
                k.mnPlaceRecognitionWords += 1
        if not sharing:
            return [], []
        maxCommonWords = max(0, max(k.mnPlaceRecognitionWords for k in sharing))
        minCommonWords = int(F32(maxCommonWords) * F32(0.8))
        scored = []
        for k in sharing:
            if self._passes_gate(k.mnPlaceRecognitionWords, minCommonWords):
                si = F32(self._score(q_ids, q_vals, k))
                k.mPlaceRecognitionScore = si
                scored.append((si, k))
        if not scored:
            return [], []
        acc_list = []
        for si, k in scored:
            bestScore = si
            best = k
            seen = [k2 for k2 in k.covis if self._same_query(k2.mnPlaceRecognitionQuery, query_kf_id)]
            accScore = self._acc_chain(si, [k2.mPlaceRecognitionScore for k2 in seen])
            for k2 in seen:
                if self._better(k2.mPlaceRecognitionScore, bestScore):
                    best = k2
                    bestScore = k2.mPlaceRecognitionScore
            acc_list.append((accScore, best))
        acc_list = self._sorted(acc_list)
        bad = set(bad_map_ids)
        loop, merge, added = [], [], set()
        i = 0
        while i < len(acc_list) and (len(loop) < nNumCandidates or len(merge) < nNumCandidates):
            k = acc_list[i][1]
            if k.mnId not in added:
                if map_id == k.map and len(loop) < nNumCandidates:
                    loop.append(k.mnId)
                elif map_id != k.map and len(merge) < nNumCandidates and k.map not in bad:
                    merge.append(k.mnId)
                added.add(k.mnId)
            i += 1
        return loop, merge
