"""The conditions the global-BA scenes (tests/gba_scenes.py) must meet, asserted on the restatement (tests/gba_reference.py)
alone: the measured spreads are the ones written down, no scene is ill-conditioned against the others, the directed scenes
do what they were built for, every other scene converges, and `included` marks the empty lists."""
import numpy as np
import pytest

import gba_reference as gr
import gba_scenes as gs

NAMES = list(gs.scenes())
DIRECTED = ("bad_pivot", "exact_start")  # their own conditions are asserted below; no convergence is asked of them


def test_tolerances_are_the_measured_ones():
    sp = gs.measure()
    for k, v in sp.items():
        # what is written down is what measures, in both directions: neither a scene that outgrew it nor a padded constant
        assert abs(v - gs.SPREAD[k]) <= 1e-9 * gs.SPREAD[k], (k, v, gs.SPREAD[k])
        assert gs.TOL[k] == 64 * gs.SPREAD[k]
    assert gs.SPREAD["pos_rel"] == 2.0 ** -23 and max(v["pos_rel"] for v in gs.scene_spreads().values()) == 0.0


@pytest.mark.parametrize("quantity", ["q", "t", "chi2_rel"])
def test_no_scene_is_ill_conditioned(quantity):
    """A scene whose spread is more than 100 times the median of the others' is to be changed, not tolerated."""
    sp = gs.scene_spreads()
    for name in NAMES:
        others = [v[quantity] for n, v in sp.items() if n != name]
        assert sp[name][quantity] <= 100 * float(np.median(others)), name


def test_scene_shapes():
    """The sizes the solver's panel and tile make interesting are the ones the scenes have."""
    W, T = gs.PANEL, gs.TILE
    rows = {n: 6 * r["n_opt_kf"] for n, r in gs.references().items()}
    assert (rows["rows_42"], rows["rows_48"], rows["rows_54"]) == (W - 6, W, W + 6)
    assert rows["rows_150"] == 3 * W + 6 and T < rows["rows_114"] - W < 2 * T and rows["kf_129"] == 6 * 129
    s = gs.scenes()
    assert s["initialisation"]["robust"] == 1 and s["initialisation"]["iterations"] == 20 and s["initialisation"]["fixed"].sum() == 1
    assert all(f["ur"] is None for f in s["initialisation"]["kfs"])
    assert s["no_fixed_stereo"]["fixed"].sum() == 0
    assert s["fixed_in_the_middle"]["fixed"].tolist() == [0, 0, 1, 0, 0] and s["rows_48"]["fixed"][0] == 1
    assert {(v["robust"], v["write_store"]) for v in s.values()} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    sv = s["special_vertices"]
    seen = np.bincount(sv["obs_kf"], minlength=len(sv["kfs"]))
    assert (seen[sv["fixed"] == 0] == 0).any()                       # an optimised keyframe without edges
    assert (np.diff(sv["obs_off"]) == 0).sum() == 1                   # a point with an empty list
    kf1 = sv["obs_kf"][sv["obs_off"][1]:sv["obs_off"][2]]
    assert len(kf1) and sv["fixed"][kf1].all()                        # a point seen only by the fixed keyframe


def test_directed_scenes():
    ref = gs.references()
    bad = ref["bad_pivot"]
    trials = [t for it in bad["trace"] for t in it]
    assert any(not ok2 for _, _, ok2 in trials) and any(not good for _, good, _ in trials)   # pivots fail, trials are popped
    assert bad["trials_run"] > bad["iterations_run"]
    ex = ref["exact_start"]
    assert ex["stop_reason"] == gr.STOP_TERMINATE and ex["iterations_run"] == 1 and ex["chi2_initial"] == 0.0
    assert {r["stop_reason"] for r in ref.values()} >= {gr.STOP_ITERATIONS, gr.STOP_TERMINATE, gr.STOP_BAD}


@pytest.mark.parametrize("name", [n for n in NAMES if n not in DIRECTED])
def test_scene_converges(name):
    ref = gs.references()[name]
    assert ref["ran"] == 1 and ref["chi2_final"] < ref["chi2_initial"]
    assert np.isfinite(ref["kf_out"]).all() and np.isfinite(ref["pos_out"]).all()


def test_outliers_pull_the_solution_without_the_kernel():
    """mixed_plain_20 ends at a cost several times that of mixed_robust_20's Huber cost: the reference's behaviour."""
    ref = gs.references()
    assert ref["mixed_plain_20"]["chi2_final"] > 3 * ref["mixed_robust_20"]["chi2_final"]


@pytest.mark.parametrize("name", NAMES)
def test_included_is_the_non_empty_lists(name):
    s, ref = gs.scenes()[name], gs.references()[name]
    assert (ref["included"] == (np.diff(s["obs_off"]) > 0)).all()
    empty = ref["included"] == 0
    assert (ref["pos_out"][empty] == s["store_pos"][s["slots"]][empty]).all()


def test_returns_before_optimize():
    s = gs.scenes()["rows_42"]
    r = gr.global_ba(s, stop_flag=True)
    assert r["ran"] == 0 and (r["kf_out"] == s["Tcw"].astype(np.float64)).all() and (r["included"] == 1).all()
    r = gr.global_ba(dict(s, obs_off=np.zeros_like(s["obs_off"])))
    assert r["ran"] == 0 and (r["included"] == 0).all()
