"""CPU: hand-built known answers that pin tests/kfdb_reference.py, the restatement of DBoW2's scoring and of
KeyFrameDatabase.cc the GPU database is compared against (tests/test_gpu_kfdb.py)."""
import numpy as np
import pytest

import kfdb_reference as kr


def uniform(words):
    words = list(words)
    return words, [1.0 / len(words)] * len(words)


def test_l1_score_of_a_vector_with_itself_is_one_and_of_disjoint_vectors_zero():
    ids, vals = [3, 7, 11, 40], [0.5, 0.25, 0.125, 0.125]
    assert kr.score(kr.L1_NORM, ids, vals, ids, vals) == 1.0
    assert kr.score(kr.L1_NORM, ids, vals, [1, 2, 50], [0.25, 0.25, 0.5]) == 0.0
    rng = np.random.default_rng(3)
    v = rng.random(200)
    v = v / v.sum()
    ids = np.sort(rng.choice(10 ** 6, 200, replace=False))
    assert kr.score(kr.L1_NORM, ids, v, ids, v) == pytest.approx(1.0, abs=1e-12)


def test_scores_of_every_type_on_a_hand_example():
    a = ([1, 2, 4], [0.5, 0.25, 0.25])
    b = ([2, 3, 4], [0.5, 0.25, 0.25])
    # shared words 2 (0.25 / 0.5) and 4 (0.25 / 0.25)
    assert kr.score(kr.L1_NORM, *a, *b) == -((0.25 - 0.25 - 0.5) + (0.0 - 0.25 - 0.25)) / 2.0 == 0.5
    assert kr.score(kr.DOT_PRODUCT, *a, *b) == 0.25 * 0.5 + 0.25 * 0.25
    assert kr.score(kr.L2_NORM, *a, *b) == 1.0 - np.sqrt(1.0 - 0.1875)
    assert kr.score(kr.L2_NORM, [1], [1.0], [1], [1.0]) == 1.0  # the score >= 1 clamp
    assert kr.score(kr.CHI_SQUARE, *a, *b) == 2. * (0.125 / 0.75 + 0.0625 / 0.5)
    assert kr.score(kr.BHATTACHARYYA, *a, *b) == np.sqrt(0.125) + 0.25
    assert kr.score(kr.CHI_SQUARE, [1], [0.0], [1], [0.0]) == 0.0  # vi + wi == 0: no term


def test_min_common_words_truncates_five_to_four():
    assert int(np.float32(5) * np.float32(0.8)) == 4
    db = kr.KeyFrameDatabase(kr.L1_NORM)
    db.add(1, *uniform(range(0, 5)), 0)      # 5 shared words
    db.add(2, *uniform(range(0, 4)), 0)      # 4: not more than minCommonWords = 4
    db.add(3, *uniform(range(1, 5)), 0)      # 4
    assert db.DetectRelocalizationCandidates(10, *uniform(range(0, 5)), 0) == [1]
    db.add(4, *uniform(range(0, 5)), 0)
    db.erase(2)
    db.add(2, *uniform([0, 1, 2, 3, 4]), 0)  # now 5 as well, behind 1 and 4
    assert db.DetectRelocalizationCandidates(11, *uniform(range(0, 5)), 0) == [1, 4, 2]


def test_stale_reloc_score_changes_the_best_keyframe():
    def build():
        db = kr.KeyFrameDatabase(kr.L1_NORM)
        db.add(1, *uniform(range(0, 10)), 0)   # A
        db.add(2, *uniform(range(10, 20)), 0)  # B
        db.set_covisibility(1, [2])
        return db
    q2 = uniform(list(range(0, 10)) + [10])  # shares 10 words with A, 1 with B (below minCommonWords = 8)
    fresh = build()
    assert fresh.DetectRelocalizationCandidates(101, *q2, 0) == [1]
    stale = build()
    assert stale.DetectRelocalizationCandidates(100, *uniform(range(10, 20)), 0) == [2]
    assert stale.kfs[2].mRelocScore == np.float32(1.0)
    # B takes query id 101 during the walk but is not scored: A's neighbour B keeps its score 1.0 from query 100,
    # beats A's own 10/11 and becomes the candidate
    assert stale.DetectRelocalizationCandidates(101, *q2, 0) == [2]
    assert stale.kfs[1].mRelocScore == np.float32(10 / 11)


def test_erase_and_re_add_moves_a_keyframe_to_the_back():
    db = kr.KeyFrameDatabase(kr.L1_NORM)
    for k in (1, 2, 3):
        db.add(k, [5], [1.0], 0)
    assert db.DetectRelocalizationCandidates(1, [5], [1.0], 0) == [1, 2, 3]
    db.erase(1)
    db.add(1, [5], [1.0], 0)
    assert db.DetectRelocalizationCandidates(2, [5], [1.0], 0) == [2, 3, 1]
    db.clearMap(0)
    assert db.DetectRelocalizationCandidates(3, [5], [1.0], 0) == []


def test_double_add_counts_twice_and_one_erase_removes_one_entry():
    db = kr.KeyFrameDatabase(kr.L1_NORM)
    db.add(1, *uniform(range(5)), 0)
    db.add(2, *uniform(range(5)), 0)
    db.add(1, *uniform(range(5)), 0)  # no erase in between: two entries per word
    # keyframe 1 has 10 words, 2 has 5 <= (int)(10 * 0.8f) = 8
    assert db.DetectRelocalizationCandidates(7, *uniform(range(5)), 0) == [1]
    db.erase(1)  # each list was [1, 2, 1]: the first entry of 1 goes, its second stays behind 2
    assert db.DetectRelocalizationCandidates(8, *uniform(range(5)), 0) == [2, 1]


def test_query_id_zero_finds_nothing_on_fresh_keyframes():
    db = kr.KeyFrameDatabase(kr.L1_NORM)
    db.add(1, *uniform(range(5)), 0)
    assert db.DetectRelocalizationCandidates(0, *uniform(range(5)), 0) == []
    assert db.DetectNBestCandidates(0, *uniform(range(5)), [], 0, 3) == ([], [])


def test_n_best_ties_keep_list_order_and_split_by_map():
    db = kr.KeyFrameDatabase(kr.L1_NORM)
    maps = {1: 0, 2: 1, 3: 0, 4: 1, 5: 2, 6: 0}
    for k, m in maps.items():
        db.add(k, [5, 6], [0.5, 0.5], m)
    db.add(7, [5, 6, 7], [0.25, 0.25, 0.5], 0)  # same words, lower score: sorted behind the ties
    # all of 1..6 tie at accScore 1: the stable sort keeps the list order
    loop, merge = db.DetectNBestCandidates(50, [5, 6], [0.5, 0.5], [], 0, 2, bad_map_ids=[1])
    assert (loop, merge) == ([1, 3], [5])
    loop, merge = db.DetectNBestCandidates(51, [5, 6], [0.5, 0.5], [3], 0, 2)
    assert (loop, merge) == ([1, 6], [2, 4])  # 3 is connected: excluded
    loop, merge = db.DetectNBestCandidates(52, [5, 6], [0.5, 0.5], [], 0, 10)
    assert (loop, merge) == ([1, 3, 6, 7], [2, 4, 5])


def test_n_best_connected_keyframe_words_reset_but_no_query_id():
    db = kr.KeyFrameDatabase(kr.L1_NORM)
    db.add(1, *uniform(range(4)), 0)
    db.add(2, *uniform(range(4)), 0)
    db.DetectNBestCandidates(9, *uniform(range(4)), [2], 0, 3)
    assert db.kfs[2].mnPlaceRecognitionQuery == 0 and db.kfs[2].mnPlaceRecognitionWords == 1
    assert db.kfs[1].mnPlaceRecognitionQuery == 9 and db.kfs[1].mnPlaceRecognitionWords == 4
