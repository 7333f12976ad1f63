"""The directed KeyFrameDatabase scenes of tests/kfdb_scenes.py, proven on the CPU: the restatement gives each scene's
expected results, and the restatement with the scene's ONE named mistake does not.  A scene whose mistake does not change
the answer is not a test."""
import numpy as np
import pytest

import kfdb_reference as kr
import kfdb_scenes as ks

NAMES = [s["name"] for s in ks.SCENES]


def test_every_scene_names_one_mistake_and_has_its_variant():
    assert len(set(NAMES)) == len(NAMES) >= 18
    assert set(ks.MISTAKES) == set(NAMES)
    for s in ks.SCENES:
        assert s["mistake"] and issubclass(ks.MISTAKES[s["name"]], kr.KeyFrameDatabase)
        assert ks.MISTAKES[s["name"]] is not kr.KeyFrameDatabase
        n_results = sum(1 for op in s["ops"] if op[0] in ("reloc", "nbest", "state"))
        assert n_results == len(s["expect"]) > 0


@pytest.mark.parametrize("name", NAMES)
def test_the_restatement_gives_the_expected_result(name):
    s = ks.BY_NAME[name]
    for scoring in ks.scorings_of(s):
        assert ks.run(s, ks.RefDriver(kr.KeyFrameDatabase(scoring))) == s["expect"], scoring


@pytest.mark.parametrize("name", NAMES)
def test_the_named_mistake_changes_the_result(name):
    s = ks.BY_NAME[name]
    for scoring in ks.scorings_of(s):
        got = ks.run(s, ks.RefDriver(ks.MISTAKES[name](scoring)))
        assert got != s["expect"], (s["mistake"], scoring)


def test_the_gate_needs_only_the_threshold_and_the_count_above_it():
    """int minCommonWords = maxCommonWords * 0.8f equals maxCommonWords * 4 / 5 for every count a query can reach, so a
    count exactly at the threshold and one above it are the whole boundary."""
    m = np.arange(0, 20001)
    assert np.array_equal((m.astype(np.float32) * np.float32(0.8)).astype(np.int64), m * 4 // 5)


def test_the_chosen_scores_are_what_the_scenes_say():
    for scoring in (kr.L1_NORM, kr.DOT_PRODUCT):
        for x in (1.0, 0.75, ks.NEXT_075, 0.5, 1 / 64, ks.EPS24, 0.0):
            assert kr.score(scoring, [5], [1.0], [5], [x]) == x
    one, e = np.float32(1), np.float32(ks.EPS24)
    assert np.float32(np.float32(one + e) + e) == one and np.float32(np.float32(e + e) + one) > one
    assert np.float32(ks.NEXT_075) > np.float32(0.75) * np.float32(1.0)
